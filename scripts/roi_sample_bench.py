"""What the proposal-target layer costs and what it saves, timed in ONE process with HIP events, the variants interleaved round by
round (median and minimum over the rounds; 5 rounds by default).  B = 8, G = 42 (30 of them gt boxes), C = 21.

    sample R / targets R     sample_roi_targets' launch (rpn_roi_sample_targets, add_gt, S = 256) beside calculate_roi_targets'
                             (rpn_roi_targets) on the same RoIs, R in {300, 2000}
    pool (8, 2000) / (8, 256)  roi_pooling forward + backward (rpn_roi_pool + rpn_roi_pool_backward), (7, 7) bins of a 32 x 32 x 512
                             map: every proposal of the 2000-proposal recipe against the sampled rows
    head M = 2400 / 2048     the f16x3-compiled head's forward + backward (7 x 7 x 512 -> 4096 -> 4096 -> 21 + 84): the 8 x 300
                             unsampled rows against the 8 x 256 sampled ones

No time is a pass mark.  Prints one table and, last, one JSON line.  Needs a GPU (there is no CPU path).
    python scripts/roi_sample_bench.py [--rounds 5] [--iters 10] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models import DetectionHead  # noqa: E402
from tf_rpn_amd.utils import roi_utils  # noqa: E402

B, G, C = 8, 42, 21
TOTAL_POS, TOTAL_NEG = 128, 128
S = TOTAL_POS + TOTAL_NEG
VARIANCES = [0.1, 0.1, 0.2, 0.2]
FEATURE = (32, 32, 512)


def time_variants(variants, rounds, iters):
    """{name: callable} -> {name: (median_us, min_us)}; each round times every variant once (iters calls between two events)."""
    for fn in variants.values():
        for _ in range(2):
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
    """30 gt boxes per image; RoIs are jittered or shifted gt boxes; a tenth of the rows is padding"""
    a = rng.uniform(0.0, 0.6, size=(B, G, 2))
    gt = np.concatenate([a, a + rng.uniform(0.15, 0.4, size=(B, G, 2))], axis=-1).astype(np.float32)
    gt_labels = rng.randint(1, C, size=(B, G)).astype(np.int32)
    gt[:, 30:] = 0.0
    gt_labels[:, 30:] = -1
    pick = gt[np.arange(B)[:, None], rng.randint(0, 30, size=(B, R))]
    hw = np.concatenate([pick[..., 2:] - pick[..., :2]] * 2, axis=-1)
    jitter = np.where((np.arange(R) % 2 == 0)[None, :, None], rng.uniform(-0.08, 0.08, size=(B, R, 4)),
                      rng.uniform(0.2, 0.9, size=(B, R, 1)) * rng.choice([-1.0, 1.0], size=(B, R, 1)))
    rois = np.clip(pick + jitter * hw, 0.0, 1.0).astype(np.float32)
    cuda = lambda x: torch.from_numpy(x).cuda()
    prio = lambda n: cuda(rng.randint(1, 2 ** 31 - 1, size=(B, n)).astype(np.int32))
    return dict(rois=cuda(rois), gt=cuda(gt), gt_labels=cuda(gt_labels), valid=torch.full((B,), R - R // 10, dtype=torch.int32, device="cuda"),
                rpos=prio(R), rneg=prio(R), spos=prio(R + G), sneg=prio(R + G))


def target_variants(lib, x, R, vptr):
    stream = L.stream_ptr()
    deltas, labels = torch.empty((B, R, 4), device="cuda"), torch.empty((B, R), dtype=torch.int32, device="cuda")
    tws_bytes = int(lib.rpn_roi_targets_workspace_bytes(B, R, G))
    tws = torch.empty((tws_bytes,), dtype=torch.uint8, device="cuda")
    o_rois, o_deltas = torch.empty((B, S, 4), device="cuda"), torch.empty((B, S, 4), device="cuda")
    o_labels, o_index = (torch.empty((B, S), dtype=torch.int32, device="cuda") for _ in range(2))
    o_counts = torch.empty((B, 2), dtype=torch.int32, device="cuda")
    sws_bytes = int(lib.rpn_roi_sample_targets_workspace_bytes(B, R, G, 1))
    sws = torch.empty((sws_bytes,), dtype=torch.uint8, device="cuda")

    def targets():
        L.check(lib.rpn_roi_targets(L.ptr(x["rois"]), L.ptr(x["valid"]), L.ptr(x["gt"]), L.ptr(x["gt_labels"]), B, R, G, TOTAL_POS, TOTAL_NEG,
                                    0.5, 0.1, 0.5, vptr, L.ptr(x["rpos"]), L.ptr(x["rneg"]), L.ptr(deltas), L.ptr(labels), L.ptr(tws),
                                    tws_bytes, stream), "targets")

    def sample():
        L.check(lib.rpn_roi_sample_targets(L.ptr(x["rois"]), L.ptr(x["valid"]), L.ptr(x["gt"]), L.ptr(x["gt_labels"]), B, R, G, 1, TOTAL_POS,
                                           TOTAL_NEG, 0.5, 0.1, 0.5, vptr, L.ptr(x["spos"]), L.ptr(x["sneg"]), S, L.ptr(o_rois),
                                           L.ptr(o_labels), L.ptr(o_deltas), L.ptr(o_index), L.ptr(o_counts), L.ptr(sws), sws_bytes, stream),
                "sample")

    sample()
    return {"targets R=%d" % R: targets, "sample R=%d" % R: sample}, (o_rois, o_counts)


def pool_variant(feat, rois, valid):
    g = torch.rand((B, int(rois.shape[1]), 7, 7, FEATURE[2]), device="cuda")

    def run():
        roi_utils.roi_pooling(feat, rois, (7, 7), valid=valid)
        roi_utils.roi_pooling_backward(g, rois, feat.shape, valid=valid)

    return run


def head_variant(lib, M):
    head = DetectionHead(C, pooling_size=(7, 7), channels=FEATURE[2], hidden=(4096, 4096), max_rois=M, seed=1)
    head.compile(precision="f16x3")
    gen = torch.Generator(device="cuda").manual_seed(0)
    pooled = torch.rand((M, 7, 7, FEATURE[2]), device="cuda", generator=gen)
    logits, deltas = torch.empty((M, C), device="cuda"), torch.empty((M, 4 * C), device="cuda")
    g_logits = torch.randn((M, C), device="cuda", generator=gen) / M
    g_deltas = torch.randn((M, 4 * C), device="cuda", generator=gen) / M
    g_pooled = torch.empty_like(pooled)
    stream = L.stream_ptr()

    def run(head=head):
        L.check(lib.rpn_det_head_forward(head._h, L.ptr(pooled), M, 1, L.ptr(logits), L.ptr(deltas), stream), "head forward")
        L.check(lib.rpn_det_head_backward(head._h, L.ptr(pooled), M, L.ptr(g_logits), L.ptr(g_deltas), L.ptr(g_pooled), stream),
                "head backward")

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    L.require_gpu()
    lib = L.lib()
    rng = np.random.RandomState(0)
    _keep, vptr = L.host_floats(VARIANCES)
    variants, sampled = {}, {}
    inputs = {}
    for R in (300, 2000):
        inputs[R] = make_inputs(rng, R)
        v, sampled[R] = target_variants(lib, inputs[R], R, vptr)
        variants.update(v)
    torch.cuda.synchronize()
    counts = {R: sampled[R][1].cpu().numpy().tolist() for R in sampled}
    feat = torch.rand((B,) + FEATURE, device="cuda")
    variants["pool fwd+bwd (8, 2000)"] = pool_variant(feat, inputs[2000]["rois"], inputs[2000]["valid"])
    variants["pool fwd+bwd (8, 256)"] = pool_variant(feat, sampled[2000][0], sampled[2000][1][:, 0].contiguous())
    variants["head f16x3 fwd+bwd M=2400"] = head_variant(lib, 2400)
    variants["head f16x3 fwd+bwd M=2048"] = head_variant(lib, 2048)
    res = time_variants(variants, args.rounds, args.iters)
    print("%-28s %12s %12s" % ("variant", "median us", "min us"))
    for name, v in res.items():
        print("%-28s %12.1f %12.1f" % (name, v[0], v[1]))
    line = json.dumps({"B": B, "G": G, "C": C, "S": S, "rounds": args.rounds, "iters": args.iters, "sampled_counts": counts,
                       "us_median_min": res})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
