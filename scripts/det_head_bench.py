"""Times the detection head (B = 8, R = 300 -> M = 2400 rows, C = 21) in ONE process with HIP events, the variants interleaved round
by round (median and minimum over the rounds), at the VGG16 (7 x 7 x 512) and MobileNetV2 (7 x 7 x 576) feature widths and hidden
widths 4096 and 1024:

    head forward     rpn_det_head_forward (keep = 1): fc1, fc2, cls | reg
    head forward f16x3  the same forward on an inference copy of the head at precision "f16x3" (split float16 on the 16-bit MFMA)
    head backward    rpn_det_head_backward with the gradient of the pooled features
    head adam        rpn_det_head_adam_step (one launch over all eight tensors)
    head step        forward (kept) + backward + adam on the float32 head, back to back between one pair of events
    head forward (training, f16x3) / head backward f16x3 / head adam + repack / head step f16x3
                     the same four on a second head of the same weights compiled with precision="f16x3": every product in split
                     float16, the gradients' shifts found on the device, the packed image refreshed after Adam
    fc1 wgrad f16x3 / fc1 dgrad f16x3   the two new GEMMs alone at fc1's shape (rpn_fc_wgrad_x3 / rpn_fc_dgrad_x3: test entries,
                     so a max|.| scan, a small allocation and a synchronisation are inside the events) and
    fc2 wgrad f16x3 / fc2 dgrad f16x3   the same at fc2's shape (M x H x H), beside
    fc2 wgrad f32 / fc2 dgrad f32       their float32 counterparts rpn_conv1x1_wgrad / rpn_conv1x1_dgrad, which as single-layer entries
                     take at most 4096 channels: fc1's K1 is beyond them, so the float32 comparison at fc1's size is the whole backward
    torch fwd+bwd+adam  the same four layers as torch.nn.Linear, float32, forward + backward (to the input) + torch.optim.Adam
    fc1 rpn_fc_forward  the first layer alone on the new GEMM (bias, no activation), with its TFLOP/s
    fc1 f16x3 (packed)  the first layer of the f16x3 head on its packed weights (rpn_det_head_forward_layer: bias and ReLU), events
                        around that one launch -- not the re-packing test entry rpn_fc_forward_x3
    fc1 torch.addmm     the same product through torch
    head step dropout / head step f16x3 dropout   (--dropout RATE) the training step on two more heads of the same weights with
                     DetectionHead(dropout=RATE): the dropout forward variants (one Philox evaluation per four stores) and the scaled
                     masks of the backward, timed beside the rate-0 steps in the same rounds
    fc1 rpn_conv2d      the same product as a 1 x 1 conv on an (M, 1, 1, K) tensor: the library's way before rpn_fc_forward existed
                        (a single-layer test entry: every call allocates, packs the kernel for its tiles and synchronises)

Also reports max |f16x3 - f32| of the logits and deltas and of the eight parameter gradients on the benchmark's inputs.  Prints one table and, last, one JSON line.  Needs a GPU (there is no CPU path).
    python scripts/det_head_bench.py [--rounds 5] [--iters 3] [--dropout RATE] [--json PATH]
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

B, R, C = 8, 300, 21
M = B * R
PEAK_TF, GUIDE_TF = 157.3, 122.0          # float32 matrix peak of the MI355X; an untuned LDS-tiled f32 MFMA GEMM at 4096^3


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


def bench_config(lib, channels, hidden, rounds, iters, dropout=0.0):
    K1 = 7 * 7 * channels
    head = DetectionHead(C, pooling_size=(7, 7), channels=channels, hidden=(hidden, hidden), max_rois=M, seed=1)
    gen = torch.Generator(device="cuda").manual_seed(0)
    pooled = torch.rand((B, R, 7, 7, channels), device="cuda", generator=gen)
    logits, deltas = torch.empty((B, R, C), device="cuda"), torch.empty((B, R, 4 * C), device="cuda")
    g_logits = torch.randn((B, R, C), device="cuda", generator=gen) / M
    g_deltas = torch.randn((B, R, 4 * C), device="cuda", generator=gen) / M
    g_pooled = torch.empty_like(pooled)
    stream = L.stream_ptr()
    h = head._h

    def fwd():
        L.check(lib.rpn_det_head_forward(h, L.ptr(pooled), M, 1, L.ptr(logits), L.ptr(deltas), stream), "forward")

    def bwd():
        L.check(lib.rpn_det_head_backward(h, L.ptr(pooled), M, L.ptr(g_logits), L.ptr(g_deltas), L.ptr(g_pooled), stream), "backward")

    def adam():
        L.check(lib.rpn_det_head_adam_step(h, 1e-4, 0.9, 0.999, 1e-7, stream), "adam")

    # the same layers in torch
    fc1, fc2 = torch.nn.Linear(K1, hidden, device="cuda"), torch.nn.Linear(hidden, hidden, device="cuda")
    cls, reg = torch.nn.Linear(hidden, C, device="cuda"), torch.nn.Linear(hidden, 4 * C, device="cuda")
    params = [p for m in (fc1, fc2, cls, reg) for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=1e-4, eps=1e-7)
    x_t = pooled.reshape(M, K1).clone().requires_grad_()

    def torch_step():
        opt.zero_grad(set_to_none=True)
        x_t.grad = None
        h2 = torch.relu(fc2(torch.relu(fc1(x_t))))
        torch.autograd.backward([cls(h2), reg(h2)], [g_logits.reshape(M, C), g_deltas.reshape(M, 4 * C)])
        opt.step()

    # the first layer alone
    w1 = fc1.weight.detach().t().contiguous()                  # (K1, hidden), the Dense layout
    b1 = fc1.bias.detach().clone()
    x2 = pooled.reshape(M, K1)
    out = torch.empty((M, hidden), device="cuda")

    def fc_new():
        L.check(lib.rpn_fc_forward(L.ptr(x2), L.ptr(w1), L.ptr(b1), M, K1, hidden, hidden, 0, L.ptr(out), stream), "rpn_fc_forward")

    def fc_torch():
        torch.addmm(b1, x2, w1, out=out)

    def fc_conv():
        L.check(lib.rpn_conv2d(L.ptr(x2), M, 1, 1, K1, L.ptr(w1), L.ptr(b1), 1, 1, hidden, 1, 0, 0, 1, 1, 0, 0, L.ptr(out), stream),
                "rpn_conv2d")

    # the f16x3 inference head with the same weights
    head_x3 = head.inference_copy(precision="f16x3")
    logits_x3, deltas_x3 = torch.empty_like(logits), torch.empty_like(deltas)
    out_x3 = torch.empty((M, hidden), device="cuda")

    def fwd_x3():
        L.check(lib.rpn_det_head_forward(head_x3._h, L.ptr(pooled), M, 0, L.ptr(logits_x3), L.ptr(deltas_x3), stream), "forward f16x3")

    def fc_x3():
        L.check(lib.rpn_det_head_forward_layer(head_x3._h, b"fc1", L.ptr(x2), M, L.ptr(out_x3), stream), "forward_layer f16x3")

    # a second trainable head with the same weights, compiled in f16x3
    head_t = DetectionHead(C, pooling_size=(7, 7), channels=channels, hidden=(hidden, hidden), max_rois=M, seed=1)
    head_t.compile(precision="f16x3")
    ht = head_t._h
    logits_t, deltas_t = torch.empty_like(logits), torch.empty_like(deltas)

    def fwd_t():
        L.check(lib.rpn_det_head_forward(ht, L.ptr(pooled), M, 1, L.ptr(logits_t), L.ptr(deltas_t), stream), "forward (training, f16x3)")

    def bwd_t():
        L.check(lib.rpn_det_head_backward(ht, L.ptr(pooled), M, L.ptr(g_logits), L.ptr(g_deltas), L.ptr(g_pooled), stream), "backward f16x3")

    def adam_t():
        L.check(lib.rpn_det_head_adam_step(ht, 1e-4, 0.9, 0.999, 1e-7, stream), "adam + repack")

    def step():
        fwd(), bwd(), adam()

    def step_t():
        fwd_t(), bwd_t(), adam_t()

    # --dropout: two more trainable heads of the same weights, float32 and f16x3, at that rate
    drop_steps = {}
    if dropout > 0.0:
        for name, precision in (("head step dropout", "f32"), ("head step f16x3 dropout", "f16x3")):
            hd = DetectionHead(C, pooling_size=(7, 7), channels=channels, hidden=(hidden, hidden), max_rois=M, seed=1, dropout=dropout)
            hd.compile(precision=precision)
            lo, de = torch.empty_like(logits), torch.empty_like(deltas)

            def step_d(hd=hd, lo=lo, de=de, name=name):
                L.check(lib.rpn_det_head_forward(hd._h, L.ptr(pooled), M, 1, L.ptr(lo), L.ptr(de), stream), name)
                L.check(lib.rpn_det_head_backward(hd._h, L.ptr(pooled), M, L.ptr(g_logits), L.ptr(g_deltas), L.ptr(g_pooled), stream), name)
                L.check(lib.rpn_det_head_adam_step(hd._h, 1e-4, 0.9, 0.999, 1e-7, stream), name)

            drop_steps[name] = step_d

    # the two new GEMMs alone at fc1's shape, and their float32 counterparts
    g_h1 = torch.randn((M, hidden), device="cuda", generator=gen) / M
    dw1, dx1 = torch.empty((K1, hidden), device="cuda"), torch.empty((M, K1), device="cuda")
    w2 = fc2.weight.detach().t().contiguous()
    h1 = torch.rand((M, hidden), device="cuda", generator=gen)
    dw2, dx2 = torch.empty((hidden, hidden), device="cuda"), torch.empty((M, hidden), device="cuda")
    ws_bytes_w = int(lib.rpn_conv1x1_wgrad_workspace_bytes(M, hidden, hidden))
    ws_w = torch.empty((max(ws_bytes_w, 4) // 4,), device="cuda")

    def wgrad_x3():
        L.check(lib.rpn_fc_wgrad_x3(L.ptr(x2), L.ptr(g_h1), M, K1, hidden, hidden, hidden, L.ptr(dw1), None, stream), "rpn_fc_wgrad_x3")

    def dgrad_x3():
        L.check(lib.rpn_fc_dgrad_x3(L.ptr(g_h1), L.ptr(w1), M, K1, hidden, hidden, hidden, None, L.ptr(dx1), None, stream), "rpn_fc_dgrad_x3")

    def wgrad2_x3():
        L.check(lib.rpn_fc_wgrad_x3(L.ptr(h1), L.ptr(g_h1), M, hidden, hidden, hidden, hidden, L.ptr(dw2), None, stream), "rpn_fc_wgrad_x3")

    def dgrad2_x3():
        L.check(lib.rpn_fc_dgrad_x3(L.ptr(g_h1), L.ptr(w2), M, hidden, hidden, hidden, hidden, None, L.ptr(dx2), None, stream), "rpn_fc_dgrad_x3")

    def wgrad2_f32():
        L.check(lib.rpn_conv1x1_wgrad(L.ptr(h1), L.ptr(g_h1), M, hidden, hidden, L.ptr(dw2), L.ptr(ws_w), ws_bytes_w, stream), "rpn_conv1x1_wgrad")

    def dgrad2_f32():
        L.check(lib.rpn_conv1x1_dgrad(L.ptr(g_h1), L.ptr(w2), None, M, hidden, hidden, L.ptr(dx2), stream), "rpn_conv1x1_dgrad")

    # max |f16x3 - f32| of the eight gradients, before any Adam step has moved the two heads apart
    fwd(), bwd(), fwd_t(), bwd_t()
    torch.cuda.synchronize()
    g32, g16 = head.get_gradients(), head_t.get_gradients()
    grad_diff = {"%s/%s" % (n, k): [float(np.abs(g16[n][k].astype(np.float64) - g32[n][k]).max()), float(np.abs(g32[n][k]).max())]
                 for n in g32 for k in g32[n]}
    grad_range = head_t.status()["f16_range"]

    fwd()
    fwd_x3()
    torch.cuda.synchronize()
    diff = {"logits": float((logits_x3 - logits).abs().max()), "deltas": float((deltas_x3 - deltas).abs().max()),
            "max_abs_logits": float(logits.abs().max()), "max_abs_deltas": float(deltas.abs().max()),
            "f16_range": head_x3.status()["f16_range"]}

    variants = {"head forward f16x3": fwd_x3, "fc1 f16x3 (packed)": fc_x3, "head forward": fwd, "head backward": bwd, "head adam": adam, "torch fwd+bwd+adam": torch_step, "fc1 rpn_fc_forward": fc_new,
                "fc1 torch.addmm": fc_torch, "head forward (training, f16x3)": fwd_t, "head backward f16x3": bwd_t,
                "head adam + repack": adam_t, "head step": step, "head step f16x3": step_t, "fc1 wgrad f16x3": wgrad_x3,
                "fc1 dgrad f16x3": dgrad_x3, "fc2 wgrad f32": wgrad2_f32, "fc2 wgrad f16x3": wgrad2_x3, "fc2 dgrad f32": dgrad2_f32,
                "fc2 dgrad f16x3": dgrad2_x3}
    variants.update(drop_steps)
    # the backward needs a kept forward; every timed backward reuses the last one, so in every round each head's forward comes before
    # its backward and its adam (which drops the kept forward) after it
    fwd()
    fwd_t()
    conv_note = None
    try:
        fc_conv()
        conv = out.clone()
        fc_new()
        conv_note = "max |rpn_conv2d - rpn_fc_forward| = %.3e" % float((conv - out).abs().max())
        variants["fc1 rpn_conv2d"] = fc_conv
    except (ValueError, RuntimeError) as e:
        conv_note = "rpn_conv2d refuses this shape: %s" % e
    order = ["head forward", "head forward f16x3", "head forward (training, f16x3)", "head backward", "head backward f16x3", "head adam",
             "head adam + repack", "head step", "head step dropout", "head step f16x3", "head step f16x3 dropout", "torch fwd+bwd+adam", "fc1 rpn_fc_forward", "fc1 f16x3 (packed)",
             "fc1 torch.addmm", "fc1 wgrad f16x3", "fc1 dgrad f16x3", "fc2 wgrad f32", "fc2 wgrad f16x3", "fc2 dgrad f32", "fc2 dgrad f16x3",
             "fc1 rpn_conv2d"]
    variants = {n: variants[n] for n in order if n in variants}
    res = time_variants(variants, rounds, iters)
    flop1 = 2.0 * M * K1 * hidden
    tf = {n: flop1 / (res[n][0] * 1e-6) / 1e12 for n in res if n.startswith("fc1")}
    tf.update({n: 2.0 * M * hidden * hidden / (res[n][0] * 1e-6) / 1e12 for n in res if n.startswith("fc2")})
    w_bytes, ws_bytes = head.memory_bytes()
    x3_bytes = head_x3.memory_bytes()
    spread = lambda n: (res[n][2] - res[n][1]) / res[n][0]      # (max - min) / median over the rounds
    train = dict(step_f32_over_f16x3=res["head step"][0] / res["head step f16x3"][0],
                 step_f16x3_over_torch=res["head step f16x3"][0] / res["torch fwd+bwd+adam"][0],
                 step_spread_f32=spread("head step"), step_spread_f16x3=spread("head step f16x3"), grad_max_abs_diff_and_max_abs=grad_diff,
                 grad_f16_range=grad_range, train_weights_bytes=head_t.memory_bytes()[0], train_workspace_bytes=head_t.memory_bytes()[1])
    if drop_steps:
        train.update(dropout_rate=dropout, step_dropout_over_rate0_f32=res["head step dropout"][0] / res["head step"][0],
                     step_dropout_over_rate0_f16x3=res["head step f16x3 dropout"][0] / res["head step f16x3"][0])
    return dict(us_median_min=res, fc1_tflops=tf, f16x3_training=train, conv_note=conv_note, weights_bytes=w_bytes, workspace_bytes=ws_bytes,
                f16x3_weights_bytes=x3_bytes[0], f16x3_workspace_bytes=x3_bytes[1], f16x3_minus_f32=diff,
                f16x3_forward_speedup=res["head forward"][0] / res["head forward f16x3"][0],
                f16x3_fc1_speedup=res["fc1 rpn_fc_forward"][0] / res["fc1 f16x3 (packed)"][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.0, help="also time the training step at this dropout rate (0: no such leg)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    L.require_gpu()
    lib = L.lib()
    results = {}
    for backbone, channels in (("vgg16", 512), ("mobilenet_v2", 576)):
        for hidden in (4096, 1024):
            label = "%s K1=%d H=%d" % (backbone, 49 * channels, hidden)
            results[label] = bench_config(lib, channels, hidden, args.rounds, args.iters, args.dropout)
            torch.cuda.empty_cache()
    print("%-32s %-30s %12s %12s %10s" % ("shape (M = %d)" % M, "variant", "median us", "min us", "TFLOP/s"))
    for label, row in results.items():
        for name, v in row["us_median_min"].items():
            tf = row["fc1_tflops"].get(name)
            print("%-32s %-30s %12.1f %12.1f %10s" % (label, name, v[0], v[1], "%.1f" % tf if tf else ""))
        print("%-32s %s" % (label, row["conv_note"]))
        t = row["f16x3_training"]
        worst = max(t["grad_max_abs_diff_and_max_abs"].items(), key=lambda kv: kv[1][0] / max(kv[1][1], 1e-300))
        print("%-32s training step f32 / f16x3 %.2fx (spread of the rounds: f32 %.1f %%, f16x3 %.1f %%); f16x3 step / torch step %.2f; max "
              "|f16x3 - f32| of the gradients, worst relative to max |g|: %s %.3e of %.3e; range flag %s; weights %.0f MB" % (
                  label, t["step_f32_over_f16x3"], 100 * t["step_spread_f32"], 100 * t["step_spread_f16x3"], t["step_f16x3_over_torch"],
                  worst[0], worst[1][0], worst[1][1], t["grad_f16_range"], t["train_weights_bytes"] / 1e6))
        if "dropout_rate" in t:
            print("%-32s training step at dropout %.2f / at rate 0: f32 %.3fx, f16x3 %.3fx" % (label, t["dropout_rate"], t["step_dropout_over_rate0_f32"],
                                                                                       t["step_dropout_over_rate0_f16x3"]))
        d = row["f16x3_minus_f32"]
        print("%-32s f16x3 / f32: head forward %.2fx, fc1 %.2fx; max |f16x3 - f32| logits %.3e (max |logit| %.3e), deltas %.3e (max "
              "|delta| %.3e); range flag %s; f16x3 head weights %.0f MB" % (label, row["f16x3_forward_speedup"], row["f16x3_fc1_speedup"],
                                                                          d["logits"], d["max_abs_logits"], d["deltas"], d["max_abs_deltas"],
                                                                          d["f16_range"], row["f16x3_weights_bytes"] / 1e6))
    print("float32 matrix peak %.1f TFLOP/s; untuned LDS-tiled f32 MFMA GEMM (4096^3) %.1f TFLOP/s" % (PEAK_TF, GUIDE_TF))
    line = json.dumps({"B": B, "R": R, "C": C, "rounds": args.rounds, "iters": args.iters, "dropout": args.dropout, "peak_tflops": PEAK_TF, "guide_tflops": GUIDE_TF,
                       "results": results})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
