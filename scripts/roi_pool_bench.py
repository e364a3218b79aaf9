"""Times RoI pooling at the workload's shape (B = 8, R = 300, 7 x 7) in ONE process with HIP events, the variants interleaved
round by round (median and minimum over the rounds):

    per feature map (VGG16 31 x 31 x 512, MobileNetV2 32 x 32 x 576, random float32 data, random boxes inside the image):
      forward f32        rpn_roi_pool
      backward           rpn_roi_pool_backward
      torch gather       the same bilinear arithmetic written with torch advanced indexing, same device
      zero_ fill         torch.Tensor.zero_() on an output-sized tensor: the store-bound floor the forward is judged against
      align s=N ...      rpn_roi_align / rpn_roi_align_backward at sampling ratio N = 1, 2 and the default extent (same boxes, same
                         output bytes; 4 N^2 corner loads per store instead of 4)
      max forward f32    rpn_roi_max_pool without the argmax (inference: the same output bytes; a bin of a large box reads
                         about 20 pixels per store where the bilinear pool reads 4), at the default extent (H - 1, W - 1)
      max forward+argmax the same with the int32 argmax stored beside it (training: twice the bytes written)
      max backward       rpn_roi_max_pool_backward with that argmax
      crop14 + max2x2    rpn_roi_pool at 14 x 14 followed by torch.nn.functional.max_pool2d(2): what a user had to do for
                         max-pooled RoI features before (writes and re-reads a 4x larger intermediate)
    per backbone at precision f16x3, 500 x 500 images, after one forward (the tap as the graph leaves it in the arena):
      model pool         rpn_model_roi_pool (VGG16: the split hi / lo form; MobileNetV2's tap is float32 in every precision)
      tap copy           rpn_model_get_activation of the tap (VGG16: the split_to_f32 launch the split instantiation replaces)
      forward f32        rpn_roi_pool on that copy
      align s=N model    rpn_model_roi_align (the split form where the tap is kept in it)
      max model          rpn_model_roi_max_pool, no argmax

Prints one table and, last, one JSON line.  Needs a GPU (there is no CPU path).
    python scripts/roi_pool_bench.py [--rounds 20] [--iters 20] [--json PATH]
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

B, R, PH, PW = 8, 300, 7, 7
ALIGN_S = (1, 2)            # RoI Align's sampling ratios timed beside the pool


def torch_gather_pool(x, rois, ph, pw):
    """crop_and_resize(bilinear, extrapolation 0) with torch ops: the plain restatement a user would write (ph, pw > 1)."""
    Bn, H, W, C = x.shape
    ky = torch.arange(ph, device=x.device, dtype=torch.float32)
    kx = torch.arange(pw, device=x.device, dtype=torch.float32)
    in_y = (rois[..., 0] * (H - 1))[..., None] + ky * ((rois[..., 2] - rois[..., 0]) * (H - 1) / (ph - 1))[..., None]     # (B,R,ph)
    in_x = (rois[..., 1] * (W - 1))[..., None] + kx * ((rois[..., 3] - rois[..., 1]) * (W - 1) / (pw - 1))[..., None]     # (B,R,pw)
    oky, okx = (in_y >= 0) & (in_y <= H - 1), (in_x >= 0) & (in_x <= W - 1)
    in_y, in_x = in_y.clamp(0, H - 1), in_x.clamp(0, W - 1)
    t, l = in_y.floor(), in_x.floor()
    ly, lx = (in_y - t)[..., :, None, None], (in_x - l)[..., None, :, None]
    t, bt, l, rt = t.long(), in_y.ceil().long(), l.long(), in_x.ceil().long()
    bi = torch.arange(Bn, device=x.device)[:, None, None, None]
    g = lambda yy, xx: x[bi, yy[..., :, None], xx[..., None, :]]                                                           # (B,R,ph,pw,C)
    top = g(t, l) + (g(t, rt) - g(t, l)) * lx
    bot = g(bt, l) + (g(bt, rt) - g(bt, l)) * lx
    return (top + (bot - top) * ly) * (oky[..., :, None] & okx[..., None, :])[..., None]


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


def boxes(rng, n_images):
    lo = rng.uniform(0.0, 0.7, size=(n_images, R, 2))
    hi = np.minimum(lo + rng.uniform(0.05, 0.6, size=(n_images, R, 2)), 0.98)      # (inside: no sample near the border)
    return torch.from_numpy(np.concatenate([lo, hi], axis=-1).astype(np.float32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    L.require_gpu()
    rng = np.random.RandomState(0)
    lib = L.lib()
    results = {}
    rois = boxes(rng, B)
    valid = torch.full((B,), R, dtype=torch.int32, device="cuda")
    for label, (H, W, C) in (("vgg16 31x31x512", (31, 31, 512)), ("mobilenet_v2 32x32x576", (32, 32, 576))):
        x = torch.from_numpy(rng.standard_normal((B, H, W, C)).astype(np.float32)).cuda()
        out = torch.empty((B, R, PH, PW, C), dtype=torch.float32, device="cuda")
        dy = torch.from_numpy(rng.standard_normal((B, R, PH, PW, C)).astype(np.float32)).cuda()
        dx = torch.empty_like(x)
        fill = torch.empty_like(out)
        stream = L.stream_ptr()
        want = torch_gather_pool(x, rois, PH, PW)
        L.check(lib.rpn_roi_pool(L.ptr(x), B, H, W, C, L.ptr(rois), R, PH, PW, L.ptr(valid), L.ptr(out), stream), "rpn_roi_pool")
        assert (out - want).abs().max().item() <= 1e-4 * x.abs().max().item()        # same operator (torch may contract / reorder)
        variants = {
            "forward f32": lambda: lib.rpn_roi_pool(L.ptr(x), B, H, W, C, L.ptr(rois), R, PH, PW, L.ptr(valid), L.ptr(out), stream),
            "backward": lambda: lib.rpn_roi_pool_backward(L.ptr(dy), L.ptr(rois), L.ptr(valid), B, H, W, C, R, PH, PW, L.ptr(dx), stream),
            "torch gather": lambda: torch_gather_pool(x, rois, PH, PW),
            "zero_ fill": lambda: fill.zero_(),
        }
        for s in ALIGN_S:          # (s=s: each lambda keeps its own sampling ratio)
            variants["align s=%d forward f32" % s] = lambda s=s: lib.rpn_roi_align(
                L.ptr(x), B, H, W, C, L.ptr(rois), R, PH, PW, s, float(H), float(W), L.ptr(valid), L.ptr(out), stream)
            variants["align s=%d backward" % s] = lambda s=s: lib.rpn_roi_align_backward(
                L.ptr(dy), L.ptr(rois), L.ptr(valid), B, H, W, C, R, PH, PW, s, float(H), float(W), L.ptr(dx), stream)
        argmax = torch.empty((B, R, PH, PW, C), dtype=torch.int32, device="cuda")
        out14 = torch.empty((B, R, 2 * PH, 2 * PW, C), dtype=torch.float32, device="cuda")
        nchw14 = out14.view(B * R, 2 * PH, 2 * PW, C).permute(0, 3, 1, 2)           # (a channels-last view: no copy)
        ey, ex = float(H - 1), float(W - 1)

        def crop14_then_max():
            lib.rpn_roi_pool(L.ptr(x), B, H, W, C, L.ptr(rois), R, 2 * PH, 2 * PW, L.ptr(valid), L.ptr(out14), stream)
            return torch.nn.functional.max_pool2d(nchw14, 2)

        L.check(lib.rpn_roi_max_pool(L.ptr(x), B, H, W, C, L.ptr(rois), R, PH, PW, ey, ex, L.ptr(valid), L.ptr(out), L.ptr(argmax),
                                     stream), "rpn_roi_max_pool")
        assert tuple(crop14_then_max().shape) == (B * R, C, PH, PW) and int(argmax.min()) >= 0
        variants["max forward f32"] = lambda: lib.rpn_roi_max_pool(
            L.ptr(x), B, H, W, C, L.ptr(rois), R, PH, PW, ey, ex, L.ptr(valid), L.ptr(out), None, stream)
        variants["max forward+argmax"] = lambda: lib.rpn_roi_max_pool(
            L.ptr(x), B, H, W, C, L.ptr(rois), R, PH, PW, ey, ex, L.ptr(valid), L.ptr(out), L.ptr(argmax), stream)
        variants["max backward"] = lambda: lib.rpn_roi_max_pool_backward(
            L.ptr(dy), L.ptr(argmax), L.ptr(rois), L.ptr(valid), B, H, W, C, R, PH, PW, ey, ex, L.ptr(dx), stream)
        variants["crop14 + max2x2"] = crop14_then_max
        results[label] = dict(time_variants(variants, args.rounds, args.iters), out_bytes=out.numel() * 4)
        del x, out, dy, dx, fill, want, argmax, out14, nchw14
    from tf_rpn_amd.predictor import Proposer
    for backbone in ("vgg16", "mobilenet_v2"):
        prop = Proposer(backbone, precision="f16x3", max_batch=B)
        hp = prop.hyper_params
        imgs = torch.from_numpy(rng.uniform(0, 1, size=(B, hp["img_size"], hp["img_size"], 3)).astype(np.float32)).cuda()
        prop.forward(imgs)
        model, fe = prop.rpn_model, prop.feature_extractor
        tap = fe.output()
        _, H, W, C = tap.shape
        out = torch.empty((B, R, PH, PW, C), dtype=torch.float32, device="cuda")
        assert torch.equal(fe.roi_pool(rois, (PH, PW), valid=valid), roi_utils.roi_pooling(tap, rois, (PH, PW), valid=valid))
        h, name, stream = model._h, model.tap_layer.encode(), L.stream_ptr()
        variants = {
            "model pool": lambda: lib.rpn_model_roi_pool(h, L.ptr(rois), B, R, PH, PW, L.ptr(valid), L.ptr(out), stream),
            "tap copy": lambda: lib.rpn_model_get_activation(h, name, L.ptr(tap), tap.numel() * 4, None, stream),
            "forward f32": lambda: lib.rpn_roi_pool(L.ptr(tap), B, H, W, C, L.ptr(rois), R, PH, PW, L.ptr(valid), L.ptr(out), stream),
        }
        for s in ALIGN_S:
            assert torch.equal(fe.roi_align(rois, (PH, PW), s, valid=valid), roi_utils.roi_align(tap, rois, (PH, PW), s, valid=valid))
            variants["align s=%d model" % s] = lambda s=s: lib.rpn_model_roi_align(
                h, L.ptr(rois), B, R, PH, PW, s, float(H), float(W), L.ptr(valid), L.ptr(out), stream)
        assert torch.equal(fe.roi_max_pool(rois, (PH, PW), valid=valid), roi_utils.roi_max_pooling(tap, rois, (PH, PW), valid=valid))
        variants["max model"] = lambda: lib.rpn_model_roi_max_pool(
            h, L.ptr(rois), B, R, PH, PW, float(H - 1), float(W - 1), L.ptr(valid), L.ptr(out), None, stream)
        results["%s f16x3 handle %dx%dx%d" % (backbone, H, W, C)] = dict(time_variants(variants, args.rounds, args.iters),
                                                                          out_bytes=out.numel() * 4)
        del prop, out, tap
    print("%-36s %-22s %10s %10s %9s" % ("shape", "variant", "median us", "min us", "GB/s out"))
    for label, row in results.items():
        for name, v in row.items():
            if name != "out_bytes":
                writes_out = name in ("forward f32", "model pool", "zero_ fill", "torch gather") or name.endswith(("forward f32", "model", "+argmax"))
                rate = "%9.0f" % (row["out_bytes"] / v[0] / 1e3) if writes_out else ""
                print("%-36s %-22s %10.1f %10.1f %s" % (label, name, v[0], v[1], rate))
    line = json.dumps({"B": B, "R": R, "pool": [PH, PW], "rounds": args.rounds, "iters": args.iters, "us_median_min": results})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
