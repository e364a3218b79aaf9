"""Times the device evaluator (utils/eval_utils.py, rpn_evaluator_*) in ONE process, HIP events around the device work, beside what
a user does without it:

    update             DetectionEvaluator.update at B = 8, M = 300, G = 42, C = 21 (device tensors in, no flags out)
    update_proposals   the proposal recall of the same batch, R = 300, top_k (10, 100, 300), two thresholds
    d2h + numpy        the same batch copied to the host (four .cpu() calls: a synchronisation per batch) and matched by a numpy
                       loop in score order with a `taken` array -- host wall clock
    result             rpn_evaluator_result after 4952 images (VOC2007 test) of 300 rows: ranking of 21 classes + both APs
    result + readback  DetectionEvaluator.result(): the same plus the copies to the host -- host wall clock
    torch result       the same ranking and all-point AP as torch.sort (stable) + cumsum + cummax per class on the device
    numpy result       the same on the host from the (score, class, flag) arrays, np.lexsort per class -- host wall clock

The records are synthetic (detections jittered off the gts, uniform scores), the same for every variant; the script checks that the
three APs agree before it prints.  Prints one table and, last, one JSON line.  Needs a GPU (there is no CPU path).
    python scripts/eval_bench.py [--images 4952] [--rounds 5] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.utils import eval_utils  # noqa: E402

B, M, G, C, R = 8, 300, 42, 21, 300
TOP_K, RECALL_IOU = (10, 100, 300), (0.5, 0.7)


def make_batch(rng):
    gtb = np.zeros((B, G, 4), np.float32)
    y1, x1 = rng.uniform(0, 0.7, size=(B, G)), rng.uniform(0, 0.7, size=(B, G))
    gtb[..., 0], gtb[..., 1], gtb[..., 2], gtb[..., 3] = y1, x1, y1 + rng.uniform(0.1, 0.3, size=(B, G)), x1 + rng.uniform(0.1, 0.3, size=(B, G))
    gtl = rng.randint(1, C, size=(B, G)).astype(np.int32)
    gtl[:, rng.randint(8, G):] = -1                                                      # padding rows
    gtd = (rng.uniform(size=(B, G)) < 0.15).astype(np.uint8)
    pick = rng.randint(0, G, size=(B, M))
    boxes = np.take_along_axis(gtb, pick[..., None].repeat(4, axis=2), axis=1) + rng.normal(0, 0.03, size=(B, M, 4)).astype(np.float32)
    lab = np.take_along_axis(gtl, pick, axis=1)
    classes = np.where(lab >= 1, lab, rng.randint(1, C, size=(B, M))).astype(np.float32)    # (a padding row's box: some class, a miss)
    scores = rng.uniform(0.01, 1.0, size=(B, M)).astype(np.float32)
    valid = rng.randint(M // 2, M + 1, size=(B,)).astype(np.int32)
    return [np.ascontiguousarray(a) for a in (boxes.astype(np.float32), scores, classes, valid, gtb, gtl, gtd)]


def iou_map(b, g):
    """generate_iou_map of the reference for one image: b (M,4), g (G,4) -> (M,G) float32"""
    xt, yt = np.maximum(b[:, None, 1], g[None, :, 1]), np.maximum(b[:, None, 0], g[None, :, 0])
    xb, yb = np.minimum(b[:, None, 3], g[None, :, 3]), np.minimum(b[:, None, 2], g[None, :, 2])
    inter = np.maximum(xb - xt, np.float32(0)) * np.maximum(yb - yt, np.float32(0))
    ab, ag = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (ab[:, None] + ag[None, :] - inter)


def numpy_update(boxes, scores, classes, valid, gtb, gtl, gtd, thr=np.float32(0.5)):
    """what a user writes today: per image, detections in score order against a `taken` array -> flags (B,M)"""
    flags = np.full(scores.shape, -1, np.int32)
    for b in range(scores.shape[0]):
        iou = iou_map(boxes[b], gtb[b])
        iou = np.where(gtl[b][None, :] == classes[b][:, None].astype(np.int32), iou, np.float32(-np.inf))
        jmax, best = iou.argmax(axis=1), iou.max(axis=1)
        taken = np.zeros((gtl.shape[1],), bool)
        rows = np.arange(valid[b])
        for m in rows[np.lexsort((rows, -scores[b, :valid[b]]))]:
            j = jmax[m]
            if not best[m] >= thr:
                flags[b, m] = 0
            elif gtd[b, j]:
                flags[b, m] = -1
            elif taken[j]:
                flags[b, m] = 0
            else:
                taken[j], flags[b, m] = True, 1
    return flags


def numpy_result(scores, classes, flags, npos):
    ap = np.full((C,), np.nan)
    slot = np.arange(scores.size)
    for c in range(1, C):
        if npos[c] == 0:
            continue
        sel = (classes == c) & (flags >= 0)
        order = np.lexsort((slot[sel], -scores[sel].astype(np.float64)))
        tp = flags[sel][order]
        cum = np.cumsum(tp)
        prec = cum / np.arange(1, len(tp) + 1, dtype=np.float64)
        pmax = np.maximum.accumulate(prec[::-1])[::-1]
        ap[c] = pmax[tp == 1].sum() / npos[c]
    return ap


def torch_result(scores, classes, flags, npos):
    ap = torch.full((C,), float("nan"), dtype=torch.float64, device="cuda")
    for c in range(1, C):
        sel = (classes == c) & (flags >= 0)
        s, tp = scores[sel], flags[sel]
        order = torch.sort(s, descending=True, stable=True).indices
        tp = tp[order].to(torch.float64)
        cum = torch.cumsum(tp, 0)
        prec = cum / torch.arange(1, tp.numel() + 1, dtype=torch.float64, device="cuda")
        pmax = torch.cummax(prec.flip(0), 0).values.flip(0)
        ap[c] = (pmax * tp).sum() / npos[c]
    return ap


def device_us(fn, rounds, iters=1):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return float(np.median(out)), float(np.min(out))


def host_us(fn, rounds):
    fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    L.require_gpu()
    lib = L.lib()
    images = (args.images // B) * B
    rng = np.random.RandomState(0)
    pool = [make_batch(rng) for _ in range(16)]
    dev = [[torch.from_numpy(a).cuda() for a in batch] for batch in pool]
    rois = [d[0].clone() for d in dev]
    ev = eval_utils.DetectionEvaluator(C, images + 64 * B, M, top_k=TOP_K, recall_iou=RECALL_IOU)
    res = {}

    # ---- one batch --------------------------------------------------------------------------------------------------------
    turn = [0]

    def update():
        if ev.images + B > ev.max_images:
            ev.reset()
        d = dev[turn[0] % 16]
        turn[0] += 1
        ev.update(*d, return_flags=False)

    def proposals():
        d = dev[turn[0] % 16]
        turn[0] += 1
        ev.update_proposals(rois[turn[0] % 16], d[3], d[4], d[5], d[6])

    def host_way():
        d = dev[turn[0] % 16]
        turn[0] += 1
        numpy_update(*[t.cpu().numpy() for t in d])

    res["update"] = device_us(update, args.rounds, iters=32)
    res["update_proposals"] = device_us(proposals, args.rounds, iters=32)
    res["d2h + numpy"] = host_us(host_way, args.rounds)
    same = all(np.array_equal(numpy_update(*pool[i]), eval_utils.DetectionEvaluator(C, B, M).update(*pool[i])) for i in range(2))

    # ---- a whole test set -------------------------------------------------------------------------------------------------
    ev.reset()
    flags = []
    for i in range(images // B):
        flags.append(ev.update(*dev[i % 16]))
    flags = torch.cat(flags).reshape(-1)
    scores = torch.cat([dev[i % 16][1] for i in range(images // B)]).reshape(-1)
    classes = torch.cat([dev[i % 16][2] for i in range(images // B)]).reshape(-1).to(torch.int32)
    full = ev.result()
    npos_d = torch.from_numpy(full["npos"].astype(np.float64)).cuda()
    out_ap = torch.empty((2, C), dtype=torch.float64, device="cuda")
    stream = L.stream_ptr()

    def result_device():
        L.check(lib.rpn_evaluator_result(ev._h, L.ptr(out_ap[0]), L.ptr(out_ap[1]), None, None, None, None, stream), "result")

    res["result"] = device_us(result_device, args.rounds)
    res["result + readback"] = host_us(ev.result, args.rounds)
    res["torch result"] = device_us(lambda: torch_result(scores, classes, flags, npos_d), args.rounds)
    s_h, c_h, f_h = scores.cpu().numpy(), classes.cpu().numpy(), flags.cpu().numpy()
    res["numpy result"] = host_us(lambda: numpy_result(s_h, c_h, f_h, full["npos"]), max(1, args.rounds // 2))
    ap_t, ap_n = torch_result(scores, classes, flags, npos_d).cpu().numpy(), numpy_result(s_h, c_h, f_h, full["npos"])
    err_t, err_n = float(np.nanmax(np.abs(ap_t - full["ap"]))), float(np.nanmax(np.abs(ap_n - full["ap"])))

    print("B = %d, M = %d, G = %d, C = %d; result after %d images = %d rows, %d TP + FP records; evaluator memory %.1f MB"
          % (B, M, G, C, images, images * M, int(full["ndet"].sum()), ev.memory_bytes() / 1e6))
    print("%-20s %14s %14s" % ("variant", "median us", "min us"))
    for name, (med, lo) in res.items():
        print("%-20s %14.1f %14.1f" % (name, med, lo))
    print("flags equal to the numpy loop: %s; mAP %.6f; max |AP - torch| %.3e, max |AP - numpy| %.3e" % (same, full["mAP"], err_t, err_n))
    line = json.dumps({"B": B, "M": M, "G": G, "C": C, "images": images, "records": int(full["ndet"].sum()), "rounds": args.rounds,
                       "us_median_min": res, "flags_equal": bool(same), "mAP": full["mAP"], "ap_err_torch": err_t, "ap_err_numpy": err_n,
                       "memory_bytes": ev.memory_bytes()})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)
    assert same and err_t < 1e-9 and err_n < 1e-9


if __name__ == "__main__":
    main()
