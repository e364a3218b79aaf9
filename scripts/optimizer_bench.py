"""Times the optimizer's launches (include/rpn_hip.h, "Optimizers") on caller buffers in ONE process with HIP events, the variants
interleaved round by round (median, minimum and maximum over the rounds), at two flat sizes:

    head    the detection head's buffer at 25 088 x 4096 x 4096, C = 21 (about 120 M floats; 4098 decayed ranges: the padded pair
            contributes one per row)
    vgg16   the whole-model VGG16 trainer's (about 17 M floats; 15 decayed ranges)

    adam                 rpn_optimizer_apply(ADAM, no ranges, no scale): adam_kernel, the launch both handles make by default
    adam + decay + clip  the norm pass (two launches) + optim_apply_kernel<ADAM> with the handle's range table and the scale
    sgd momentum         optim_apply_kernel<SGD>, momentum 0.9, no ranges, no scale
    sgd + decay + clip   the norm pass + optim_apply_kernel<SGD> with the range table and the scale
    norm                 rpn_grad_sq_norm alone

GB/s counts the bytes each variant must move per element ("Optimizers": Adam 28 B, SGD 20 B, the norm pass 4 B more)
and stands beside the device-to-device copy rate of profiles/r06_bw_probe.txt at the nearest size.  No time is a pass mark.
Prints one table and, last, one JSON line.  Needs a GPU (there is no CPU path).
    python scripts/optimizer_bench.py [--rounds 5] [--iters 3] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models import DetectionHead  # noqa: E402
from tf_rpn_amd.models._rpn_model import RPNModel  # noqa: E402

ADAM, SGD = 0, 1
COPY_TBS = {"head": 5.11, "vgg16": 8.29}      # profiles/r06_bw_probe.txt: copy (r+w) at 512 MB and at 93 MB


def time_variants(variants, rounds, iters):
    """{name: callable} -> {name: (median_us, min_us, max_us)}; each round times every variant once (iters calls between two events)."""
    for fn in variants.values():
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
    return {n: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for n, v in samples.items()}


def layouts():
    """{name: (floats, decayed ranges (k, 2) int64)} from the handles' own host arithmetic (no device memory)"""
    head = DetectionHead(21, pooling_size=(7, 7), channels=512, hidden=(4096, 4096), max_rois=2400, seed=None)
    w, _ = head.memory_bytes()
    model = RPNModel("vgg16", bo.get_hyper_params("vgg16"), max_batch=1)
    model.compile(train_backbone=True)
    r, K = model.decay_ranges(), model.anchor_count
    return {"head": (w // 16, head.decay_ranges()), "vgg16": (_vgg_floats(K), r)}    # (a trainable head holds w, g, m, v: 16 bytes per float)


def _vgg_floats(K):
    convs = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512),
             (512, 512), (512, 512)]
    return 9 * 512 * 512 + 512 + 513 * 5 * K + sum(9 * a * b + b for a, b in convs)


def bench_size(lib, name, n, ranges, rounds, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn((n,), device="cuda", generator=gen)
    g = torch.randn((n,), device="cuda", generator=gen) * 1e-3
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    table = torch.from_numpy(np.ascontiguousarray(ranges, dtype=np.int64)).cuda()
    ws_bytes = lib.rpn_grad_sq_norm_workspace_bytes(n)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device="cuda")
    S = torch.zeros((1,), dtype=torch.float64, device="cuda")
    c = torch.zeros((1,), dtype=torch.float32, device="cuda")
    stream = L.stream_ptr()
    lr, clip = 1e-6, 1.0                       # (a tiny rate: the buffers keep their magnitudes over the rounds)

    def norm():
        L.check(lib.rpn_grad_sq_norm(L.ptr(g), n, clip, L.ptr(S), L.ptr(c), L.ptr(ws), ws_bytes, stream), "rpn_grad_sq_norm")

    def apply(kind, extras):
        L.check(lib.rpn_optimizer_apply(kind, L.ptr(w), L.ptr(g), L.ptr(m), L.ptr(v), n, L.ptr(table) if extras else None,
                                        len(ranges) if extras else 0, 1, lr, 0.9, 0.999, 1e-7, 0.9, 0, 5e-4 if extras else 0.0,
                                        L.ptr(c) if extras else None, stream), "rpn_optimizer_apply")

    def with_norm(kind):
        norm()
        apply(kind, True)

    variants = {"adam": lambda: apply(ADAM, False), "adam + decay + clip": lambda: with_norm(ADAM), "sgd momentum": lambda: apply(SGD, False),
                "sgd + decay + clip": lambda: with_norm(SGD), "norm": norm}
    bytes_per = {"adam": 28, "adam + decay + clip": 32, "sgd momentum": 20, "sgd + decay + clip": 24, "norm": 4}
    times = time_variants(variants, rounds, iters)
    out = {}
    print("%s: %d floats (%.0f MB per buffer), %d decayed ranges; copy rate %.2f TB/s" % (name, n, n * 4 / 1e6, len(ranges), COPY_TBS[name]))
    for k, (med, lo, hi) in times.items():
        gbs = n * bytes_per[k] / med / 1e3
        out[k] = {"median_us": med, "min_us": lo, "max_us": hi, "bytes_per_element": bytes_per[k], "gb_per_s": gbs}
        print("  %-20s median %9.1f us  [%9.1f, %9.1f]  %2d B/element  %7.0f GB/s" % (k, med, lo, hi, bytes_per[k], gbs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    L.require_gpu()
    lib = L.lib()
    result = {}
    for name, (n, ranges) in layouts().items():
        result[name] = dict(bench_size(lib, name, n, ranges, args.rounds, args.iters), floats=n, ranges=len(ranges),
                            copy_tb_per_s=COPY_TBS[name])
    line = json.dumps({"optimizer_bench": result})
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
