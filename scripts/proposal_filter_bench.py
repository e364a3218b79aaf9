"""Times bbox_utils.decode_and_nms with and without the proposal filter (pre_nms_topn, min_size) -- per API call, allocations of the
outputs included -- and the filter alone -- the raw rpn_proposal_filter entry on preallocated buffers -- in ONE process, HIP events
around the device work, the variants interleaved inside every round, median of the rounds:

    (B, A, M) = (8, 8649, 300), (8, 8649, 2000)     VGG16 at 500 x 500          (pre_nms_topn 12000 cuts nothing there: the
                (1, 61440, 300), (8, 61440, 2000)    MobileNetV2 at 1024 x 1024   pre-pass's bare cost)
    pre_nms_topn in {6000, 12000}, min_size off and 16 / img_size, IoU threshold 0.7

The inputs are what the other NMS timing scripts use (scripts/nms_probe.py, scripts/bench_bbox.py; those run at import, so their
recipe is restated here): the configuration's own anchor grid, deltas ~ N(0, 1) (x variances in the kernel), scores ~ U[0, 1).
Prints one table (the README's, between the `proposal filter bench` markers) and, last, one JSON line.  Needs a GPU (there is no CPU
path).  None of the times is a pass mark.
    python scripts/proposal_filter_bench.py [--rounds 5] [--iters 20] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.utils import bbox_utils, train_utils  # noqa: E402

VARIANCES = [0.1, 0.1, 0.2, 0.2]
IOU = 0.7
GRIDS = {8649: ("vgg16", dict(img_size=500, feature_map_shape=31, anchor_ratios=[1., 2., .5])),
         61440: ("mobilenet_v2", dict(img_size=1024, feature_map_shape=64, anchor_ratios=[1., 2., .5, 3., 1 / 3.]))}
SHAPES = [(8, 8649, 300), (8, 8649, 2000), (1, 61440, 300), (8, 61440, 2000)]
TOPN = (6000, 12000)


def make_inputs(rng, B, A):
    backbone, kw = GRIDS[A]
    hp = dict(train_utils.get_hyper_params(backbone, **kw))
    anchors = bbox_utils.generate_anchors(hp)
    assert int(anchors.shape[0]) == A
    deltas = torch.from_numpy(rng.standard_normal((B, A, 4)).astype(np.float32)).cuda()
    scores = torch.from_numpy(rng.uniform(0, 1, size=(B, A)).astype(np.float32)).cuda()
    return anchors, deltas, scores, int(hp["img_size"])


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
    for B, A, M in SHAPES:
        anchors, deltas, scores, img = make_inputs(rng, B, A)
        variants = [(n, m) for n in TOPN for m in (None, 16.0 / img)]
        fns = {"nms": lambda: bbox_utils.decode_and_nms(anchors, deltas, scores, VARIANCES, M, iou_threshold=IOU)}
        # "filter alone" is the raw rpn_proposal_filter entry on preallocated buffers (the launch and nothing else); the two
        # decode_and_nms columns are per API call, output allocations and argument checks included, as a user pays them
        masked_buf = torch.empty((B, A), dtype=torch.float32, device="cuda")
        kept_buf = torch.zeros((B,), dtype=torch.int32, device="cuda")
        _keep, vptr = L.host_floats(VARIANCES)

        def raw_filter(n, m):
            use = int(m is not None)
            st = L.lib().rpn_proposal_filter(L.ptr(anchors) if use else None, L.ptr(deltas) if use else None, vptr, L.ptr(scores), B, A,
                                             n, use, m or 0.0, m or 0.0, float("-inf"), 1, L.ptr(masked_buf), L.ptr(kept_buf), None, 0,
                                             L.stream_ptr())
            L.check(st, "rpn_proposal_filter")

        for n, m in variants:
            fns["filter %d %s" % (n, m)] = lambda n=n, m=m: raw_filter(n, m)
            fns["both %d %s" % (n, m)] = lambda n=n, m=m: bbox_utils.decode_and_nms(anchors, deltas, scores, VARIANCES, M, iou_threshold=IOU,
                                                                                    pre_nms_topn=n, min_size=m)
        us = interleaved_us(fns, args.rounds, args.iters)
        plain = fns["nms"]()
        for n, m in variants:
            masked, kept = bbox_utils.filter_proposals(anchors, deltas, scores, VARIANCES, pre_nms_topn=n, min_size=m)
            both = fns["both %d %s" % (n, m)]()
            if n >= A and m is None:                      # nothing is cut: the composition must reproduce the plain path
                same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, both))
            rows.append({"B": B, "A": A, "M": M, "pre_nms_topn": n, "min_size": m, "kept_mean": float(kept.float().mean()),
                         "valid_mean": float(both[3].float().mean()), "valid_mean_plain": float(plain[3].float().mean()),
                         "nms_us": us["nms"], "filter_us": us["filter %d %s" % (n, m)], "both_us": us["both %d %s" % (n, m)]})
    print("decode_and_nms at IoU threshold %.1f with and without the proposal filter; median (min) us of %d rounds x %d calls"
          % (IOU, args.rounds, args.iters))
    print("| B | A | M | pre_nms_topn | min_size | kept per image | proposals, plain -> filtered | decode_and_nms, no filter (API call) | "
          "rpn_proposal_filter alone (raw entry) | decode_and_nms with the filter (API call) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %d | %d | %d | %s | %.0f | %.0f -> %.0f | %.1f (%.1f) | %.1f (%.1f) | %.1f (%.1f) |"
              % (r["B"], r["A"], r["M"], r["pre_nms_topn"], "off" if r["min_size"] is None else "16 px", r["kept_mean"],
                 r["valid_mean_plain"], r["valid_mean"], *r["nms_us"], *r["filter_us"], *r["both_us"]))
    print("a filter that cuts nothing reproduces the plain path, bit for bit: %s" % same)
    line = json.dumps({"rounds": args.rounds, "iters": args.iters, "iou_threshold": IOU, "rows": rows, "no_cut_equals_plain": bool(same)})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)
    assert same


if __name__ == "__main__":
    main()
