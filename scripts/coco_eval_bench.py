"""Times the COCO-style device evaluator (utils/eval_utils.CocoEvaluator, rpn_coco_evaluator_*) in ONE process, HIP events around the
device work, on the inputs of scripts/eval_bench.py (B = 8, M = 300, G = 42, C = 21), beside the VOC evaluator and the host:

    coco update        CocoEvaluator.update, default configuration (10 thresholds x 4 area ranges, max_dets (1, 10, 100)), no flags out
    voc update         DetectionEvaluator.update of the same batch
    coco result        rpn_coco_evaluator_result after 4952 images of 300 rows: ranking of 21 classes, 840 curves
    voc result         rpn_evaluator_result after the same images
    numpy update       the numpy restatement (tests/coco_eval_ref.py) of one batch on the host -- wall clock
    numpy result       its result() after `--ref-images` images -- wall clock

The script checks the device flags and APs of the first batches against the restatement before it prints.  Prints one table and,
last, one JSON line.  Needs a GPU (there is no CPU path).
    python scripts/coco_eval_bench.py [--images 4952] [--rounds 5] [--ref-images 16] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coco_eval_ref as cr  # noqa: E402
import eval_bench as eb  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.utils import eval_utils  # noqa: E402

B, M, G, C = eb.B, eb.M, eb.G, eb.C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ref-images", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    L.require_gpu()
    lib = L.lib()
    images = (args.images // B) * B
    rng = np.random.RandomState(0)
    pool = [eb.make_batch(rng) for _ in range(16)]
    dev = [[torch.from_numpy(a).cuda() for a in batch] for batch in pool]
    coco = eval_utils.CocoEvaluator(C, images + 64 * B, M)
    voc = eval_utils.DetectionEvaluator(C, images + 64 * B, M, top_k=(), recall_iou=())
    res = {}
    turn = [0]

    def update_of(ev):
        def run():
            if ev.images + B > ev.max_images:
                ev.reset()
            d = dev[turn[0] % 16]
            turn[0] += 1
            ev.update(*d, return_flags=False)
        return run

    res["coco update"] = eb.device_us(update_of(coco), args.rounds, iters=32)
    res["voc update"] = eb.device_us(update_of(voc), args.rounds, iters=32)

    # ---- the restatement: the first batches, checked and timed --------------------------------------------------------------
    n_ref = max(1, args.ref_images // B)
    ref = cr.RefCocoEvaluator(C, M)
    small = eval_utils.CocoEvaluator(C, n_ref * B, M)
    same = True
    for i in range(n_ref):
        same = same and np.array_equal(small.update(*pool[i], return_flags=True), ref.update(*pool[i]))
    got, want = small.result(), ref.result()
    ok = ~np.isnan(want["ap"])
    err = float(np.abs(got["ap"][ok] - want["ap"][ok]).max())
    same = same and np.array_equal(np.isnan(got["ap"]), ~ok) and np.array_equal(got["ar"], want["ar"], equal_nan=True)
    res["numpy update"] = eb.host_us(lambda: cr.RefCocoEvaluator(C, M).update(*pool[0]), 1)
    res["numpy result"] = eb.host_us(ref.result, 1)

    # ---- a whole test set -----------------------------------------------------------------------------------------------------
    coco.reset()
    voc.reset()
    for i in range(images // B):
        coco.update(*dev[i % 16])
        voc.update(*dev[i % 16], return_flags=False)
    full = coco.result()
    A, T, K = 4, 10, 3
    out_ap = torch.empty((C, A, T), dtype=torch.float64, device="cuda")
    out_ar = torch.empty((C, A, T, K), dtype=torch.float64, device="cuda")
    voc_ap = torch.empty((2, C), dtype=torch.float64, device="cuda")
    stream = L.stream_ptr()

    def coco_result():
        L.check(lib.rpn_coco_evaluator_result(coco._h, L.ptr(out_ap), L.ptr(out_ar), None, None, stream), "result")

    def voc_result():
        L.check(lib.rpn_evaluator_result(voc._h, L.ptr(voc_ap[0]), L.ptr(voc_ap[1]), None, None, None, None, stream), "result")

    res["coco result"] = eb.device_us(coco_result, args.rounds)
    res["voc result"] = eb.device_us(voc_result, args.rounds)

    print("B = %d, M = %d, G = %d, C = %d; result after %d images = %d rows, %d ranked rows; evaluator memory %.1f MB"
          % (B, M, G, C, images, images * M, int(full["ndet"].sum()), coco.memory_bytes() / 1e6))
    print("%-20s %14s %14s" % ("variant", "median us", "min us"))
    for name, (med, lo) in res.items():
        print("%-20s %14.1f %14.1f" % (name, med, lo))
    print("flags and ar equal to the restatement on %d images: %s; max |ap - restatement| %.3e; AP %.6f AP50 %.6f AP75 %.6f"
          % (n_ref * B, same, err, full["AP"], full["AP50"], full["AP75"]))
    line = json.dumps({"B": B, "M": M, "G": G, "C": C, "images": images, "ranked": int(full["ndet"].sum()), "rounds": args.rounds,
                       "us_median_min": res, "equal_to_restatement": bool(same), "ap_err": err, "AP": full["AP"],
                       "stats": [float(v) for v in full["stats"]], "memory_bytes": coco.memory_bytes()})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)
    assert same and err <= 2.5e-14


if __name__ == "__main__":
    main()
