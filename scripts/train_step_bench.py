"""Milliseconds per head-training step (rpn_model.train_on_batch, trainer.py:64-69) and per kernel entry at batch 8, both backbones.

    python scripts/train_step_bench.py [--batch 8] [--steps 20] [--warmup 3]
    python scripts/train_step_bench.py --train-backbone-from block1_conv1 [--batch 8] [--steps 20] [--warmup 3]
    python scripts/train_step_bench.py --backbone mobilenet_v2 --train-backbone-from block_7_expand [--batch 8] ...
    python scripts/train_step_bench.py --backbone mobilenet_v2 --train-backbone [--batch 8] ...     (the whole model; also vgg16)
    python scripts/train_step_bench.py --train-backbone --feature-grad ...       (any backbone-training leg: + the joint step)
    python scripts/train_step_bench.py --backward-precision f16x3 [--batch 8] [--steps 10] [--warmup 2]    (VGG16, the whole model)

Times on the device with HIP events around (a) a whole training step (backbone at the handle's precision + float32 head forward,
losses, backward, Adam), (b) an evaluation step (no backward), (c) the 3x3 weight-gradient entry rpn_conv3x3_wgrad on the
step's shape (its MFMA kernel + the leaf reduction) with its rate against the 157.3 TF/s float32-MFMA peak, (d) rpn_rpn_losses.
Prints one JSON line per backbone.

With --train-backbone-from LAYER (VGG16 only): (a) and (b) for the trainer that trains LAYER and every conv above it with the head
(whole VGG16 forward in exact float32, backward down to LAYER), the step's FLOP (forward + backward, counted per layer) and its rate
against the float32-MFMA peak, and per trained conv the single-layer entries rpn_conv3x3_dgrad (with its mask) and
rpn_conv3x3_wgrad_wide on that layer's shape, timed with HIP events.  A rocprofv3 --kernel-trace --stats run of the same command
gives the per-kernel totals.

With --train-backbone: compile(train_backbone=True), every layer of the backbone trains.  VGG16: the block1_conv1 report.  MobileNetV2:
(a) and (b) for the whole-model trainer, the device memory the trainer allocated at its first step, and the three stride-2 kernels'
single-layer entries on their largest layers (block_1_depthwise: 250 x 250 x 96 in, 125 x 125 out; Conv1: 500 x 500 x 3 in, 250 x
250 x 32 out) with the bytes each must move and its rate.

With --backward-precision f16x3 (VGG16, compile(train_backbone=True)): the float32 and the f16x3 training step of the same model in
ONE process -- two trainers holding the same weights, timed with HIP events in interleaved rounds, the median of 5 rounds (as
scripts/det_head_bench.py times the head) -- and per trained conv the single-layer entries of both arithmetics side by side
(rpn_conv3x3_dgrad | rpn_conv3x3_dgrad_x3 with the mask, rpn_conv3x3_wgrad_wide | rpn_conv3x3_wgrad_wide_x3; the x3 entries include
their max scan and, for the dgrad, the weight packing), with the effective TF/s of the split-float16 ones, and "d": per layer
max|g_x3 - g_f32| / max|g_f32| of the kernel gradients of one step from the same weights and batch.

With --feature-grad (a backbone-training leg): after the plain step, in the same process and with the same HIP-event method, the step
in two halves with a fixed random second-stage gradient G (B,F,F,C) at the feature tap -- "ms_feature_grad_step":
RPNModel.forward_for_training + apply_gradients(G) (the Python surface: it also copies the tap and the head outputs to fresh tensors);
"ms_split_step" / "ms_split_step_feature_grad": rpn_head_trainer_forward + rpn_head_trainer_backward with NULL / with G, nothing
else, whose difference is what the addend costs in the first dgrad's epilogue; "feature_grad_mbytes": the B F F C 4 bytes it reads.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models import rpn_mobilenet_v2, rpn_vgg16  # noqa: E402
from tf_rpn_amd.utils import bbox_utils, train_utils  # noqa: E402

PEAK_F32_MFMA = 157.3e12
# (name, cin, cout, pool after) -- keras.applications.VGG16 up to block5_conv3
VGG16 = [("block1_conv1", 3, 64, False), ("block1_conv2", 64, 64, True), ("block2_conv1", 64, 128, False),
         ("block2_conv2", 128, 128, True), ("block3_conv1", 128, 256, False), ("block3_conv2", 256, 256, False),
         ("block3_conv3", 256, 256, True), ("block4_conv1", 256, 512, False), ("block4_conv2", 512, 512, False),
         ("block4_conv3", 512, 512, True), ("block5_conv1", 512, 512, False), ("block5_conv2", 512, 512, False),
         ("block5_conv3", 512, 512, False)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def bench(backbone, precision, B, steps, warmup):
    mod = rpn_vgg16 if backbone == "vgg16" else rpn_mobilenet_v2
    hp = train_utils.get_hyper_params(backbone)
    model, _ = mod.get_model(hp, precision=precision, max_batch=B)
    imgs, deltas, lab = step_inputs(model, hp, B)
    model.compile(learning_rate=1e-5)
    lib = L.lib()
    ms_train, ms_eval = step_times(model, imgs, deltas, lab, B, steps, warmup)
    F, K = model.feature_map_shape, model.anchor_count
    cin = 512 if backbone == "vgg16" else 576
    x = torch.randn((B, F, F, cin), device="cuda")
    dy = torch.randn((B, F, F, 512), device="cuda")
    dw = torch.empty((3, 3, cin, 512), device="cuda")
    n = lib.rpn_conv3x3_wgrad_workspace_bytes(B, F, F, cin, 512)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    ms_wgrad = timed(lambda: L.check(lib.rpn_conv3x3_wgrad(L.ptr(x), L.ptr(dy), B, F, F, cin, 512, L.ptr(dw), None, L.ptr(ws), n,
                                                           L.stream_ptr()), "rpn_conv3x3_wgrad"), steps, warmup)
    flops = 2.0 * 9 * cin * 512 * B * F * F
    A = F * F * K
    reg_pred = torch.randn((B, A, 4), device="cuda")
    cls_pred = torch.rand((B, A), device="cuda")
    out = torch.empty(2, device="cuda")
    gr, gc = torch.empty_like(reg_pred), torch.empty_like(cls_pred)
    nl = lib.rpn_rpn_losses_workspace_bytes(B, A)
    wl = torch.empty(nl, dtype=torch.uint8, device="cuda")
    ms_loss = timed(lambda: L.check(lib.rpn_rpn_losses(L.ptr(deltas), L.ptr(reg_pred), L.ptr(lab), L.ptr(cls_pred), B, A, L.ptr(out),
                                                       L.ptr(gr), L.ptr(gc), L.ptr(wl), nl, L.stream_ptr()), "rpn_rpn_losses"),
                    steps, warmup)
    return {"backbone": backbone, "precision": precision, "batch": B, "ms_train_step": round(ms_train, 4),
            "ms_eval_step": round(ms_eval, 4), "ms_wgrad": round(ms_wgrad, 4), "wgrad_gflop": round(flops / 1e9, 2),
            "wgrad_tflops": round(flops / ms_wgrad / 1e9, 2), "wgrad_frac_of_f32_mfma_peak": round(flops / ms_wgrad / 1e-3 / PEAK_F32_MFMA, 3),
            "ms_losses": round(ms_loss, 4)}


def step_inputs(model, hp, B):
    rng = np.random.RandomState(0)
    imgs = torch.from_numpy(rng.uniform(0, 1, size=(B, hp["img_size"], hp["img_size"], 3)).astype(np.float32)).cuda()
    anchors = bbox_utils.generate_anchors(hp)
    gt = np.zeros((B, 4, 4), np.float32)
    gt[:, :, :2] = rng.uniform(0, 0.5, size=(B, 4, 2))
    gt[:, :, 2:] = gt[:, :, :2] + rng.uniform(0.2, 0.5, size=(B, 4, 2))
    labels = np.ones((B, 4), np.int32)
    deltas, lab = train_utils.calculate_rpn_actual_outputs(anchors, torch.from_numpy(gt).cuda(), torch.from_numpy(labels).cuda(), hp)
    return imgs, deltas.contiguous(), lab.contiguous()


def step_times(model, imgs, deltas, lab, B, steps, warmup):
    """ms per training step (update = 1) and per evaluation step (update = 0)."""
    lib = L.lib()
    losses = torch.empty(3, device="cuda")

    def step(update):
        L.check(lib.rpn_head_trainer_step(model._t, L.ptr(imgs), B, L.ptr(deltas), L.ptr(lab), update, 1e-5, 0.9, 0.999, 1e-7,
                                          L.ptr(losses), L.stream_ptr()), "rpn_head_trainer_step")

    return timed(lambda: step(1), steps, warmup), timed(lambda: step(0), steps, warmup)


def feature_grad_times(model, imgs, deltas, lab, B, steps, warmup):
    """The joint step's legs (module docstring, --feature-grad), after the plain step in the same process."""
    lib = L.lib()
    F = model.feature_map_shape
    C = model.activation_shape(model.tap_layer)[3]
    G = torch.from_numpy((np.random.RandomState(1).standard_normal((B, F, F, C)) * 1e-4).astype(np.float32)).cuda()
    losses = torch.empty(3, device="cuda")

    def python_step():
        model.forward_for_training(imgs, (deltas, lab))
        model.apply_gradients(G)

    def abi_step(g):
        L.check(lib.rpn_head_trainer_forward(model._t, L.ptr(imgs), B, L.ptr(deltas), L.ptr(lab), 1, L.ptr(losses), L.stream_ptr()),
                "rpn_head_trainer_forward")
        L.check(lib.rpn_head_trainer_backward(model._t, L.ptr(imgs), B, L.ptr(g), *(model._opt + (L.stream_ptr(),))),
                "rpn_head_trainer_backward")

    ms_null = timed(lambda: abi_step(None), steps, warmup)
    ms_g = timed(lambda: abi_step(G), steps, warmup)
    ms_py = timed(python_step, steps, warmup)
    return {"ms_split_step": round(ms_null, 4), "ms_split_step_feature_grad": round(ms_g, 4), "ms_feature_grad_step": round(ms_py, 4),
            "feature_grad_mbytes": round(G.numel() * 4 / 1e6, 1)}


def frac(flop, ms):
    return round(flop / (ms * 1e-3) / PEAK_F32_MFMA, 3)


def bench_backbone(train_from, precision, B, steps, warmup, feature_grad=False):
    hp = train_utils.get_hyper_params("vgg16")
    model, _ = rpn_vgg16.get_model(hp, precision=precision, max_batch=B)
    imgs, deltas, lab = step_inputs(model, hp, B)
    model.compile(learning_rate=1e-5, train_backbone_from=train_from)
    ms_train, ms_eval = step_times(model, imgs, deltas, lab, B, steps, warmup)
    joint = feature_grad_times(model, imgs, deltas, lab, B, steps, warmup) if feature_grad else {}
    lib = L.lib()
    F, K = model.feature_map_shape, model.anchor_count
    first = [v[0] for v in VGG16].index(train_from)
    # FLOP: the forward of the whole model, then per trained conv its wgrad and (above the first trained one) its dgrad; rpn_conv's
    # wgrad and dgrad; the 1x1 head's two backward GEMMs
    fwd = model.flops_per_image * B
    bwd = 2.0 * 2 * 9 * 512 * 512 * B * F * F + 2.0 * 2 * 512 * 5 * K * B * F * F
    layers = []
    H = hp["img_size"]
    for i, (name, cin, cout, pool) in enumerate(VGG16):
        f = 2.0 * 9 * cin * cout * B * H * H
        if i >= first:
            bwd += f + (f if i > first else 0.0)
            x = torch.randn((B, H, H, cin), device="cuda")
            dy = torch.randn((B, H, H, cout), device="cuda")
            mask = torch.randn((B, H, H, cin), device="cuda")
            dw = torch.empty((3, 3, cin, cout), device="cuda")
            db = torch.empty((cout,), device="cuda")
            nw = lib.rpn_conv3x3_wgrad_wide_workspace_bytes(B, H, H, cin, cout)
            ws = torch.empty(nw, dtype=torch.uint8, device="cuda")
            ms_w = timed(lambda: L.check(lib.rpn_conv3x3_wgrad_wide(L.ptr(x), L.ptr(dy), B, H, H, cin, cout, L.ptr(dw), L.ptr(db),
                                                                    L.ptr(ws), nw, L.stream_ptr()), "rpn_conv3x3_wgrad_wide"),
                         steps, warmup)
            row = {"layer": name, "H": H, "cin": cin, "cout": cout, "gflop": round(f / 1e9, 2), "ms_wgrad": round(ms_w, 4),
                   "wgrad_frac_of_f32_mfma_peak": frac(f, ms_w)}
            if i > first:
                dx = torch.empty((B, H, H, cin), device="cuda")
                nd = lib.rpn_conv3x3_dgrad_workspace_bytes(cin, cout)
                wsd = torch.empty(nd, dtype=torch.uint8, device="cuda")
                ms_d = timed(lambda: L.check(lib.rpn_conv3x3_dgrad(L.ptr(dy), L.ptr(dw), L.ptr(mask), B, H, H, cin, cout, L.ptr(dx),
                                                                   L.ptr(wsd), nd, L.stream_ptr()), "rpn_conv3x3_dgrad"),
                             steps, warmup)
                row.update({"ms_dgrad": round(ms_d, 4), "dgrad_frac_of_f32_mfma_peak": frac(f, ms_d)})
            layers.append(row)
            del x, dy, mask, ws
        if pool:
            H //= 2
    total = fwd + bwd
    return dict({"backbone": "vgg16", "train_backbone_from": train_from, "precision": precision, "batch": B,
                 "ms_train_step": round(ms_train, 3), "ms_eval_step": round(ms_eval, 3), "step_tflop": round(total / 1e12, 3),
                 "step_tflops": round(total / (ms_train * 1e-3) / 1e12, 2), "step_frac_of_f32_mfma_peak": frac(total, ms_train),
                 "layers": layers}, **joint)


def median_rounds(fns, steps, warmup, rounds=5):
    """{name: median over `rounds` of the ms per call}, the functions timed in turn inside every round (interleaved)"""
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            got[k].append(timed(fn, steps, warmup if r == 0 else 1))
    return {k: float(np.median(v)) for k, v in got.items()}


def bench_backward_x3(precision, B, steps, warmup):
    """module docstring, --backward-precision f16x3"""
    hp = train_utils.get_hyper_params("vgg16")
    lib = L.lib()
    models = {}
    for bp in ("f32", "f16x3"):
        model, _ = rpn_vgg16.get_model(hp, precision=precision, max_batch=B)
        model.compile(learning_rate=1e-5, train_backbone=True, backward_precision=bp)
        models[bp] = model
    imgs, deltas, lab = step_inputs(models["f32"], hp, B)
    losses = torch.empty(3, device="cuda")

    def step(model):
        L.check(lib.rpn_head_trainer_step(model._t, L.ptr(imgs), B, L.ptr(deltas), L.ptr(lab), 1, 1e-5, 0.9, 0.999, 1e-7, L.ptr(losses),
                                          L.stream_ptr()), "rpn_head_trainer_step")

    # one step each from the same weights: the per-layer distance of the gradients, and the losses, which must agree exactly
    grads, first = {}, {}
    for bp, model in models.items():
        step(model)
        torch.cuda.synchronize()
        first[bp] = losses.cpu().numpy().copy()
        grads[bp] = model.get_gradients()
    assert first["f32"].tobytes() == first["f16x3"].tobytes(), "the two steps' losses differ"
    d = {name: float(np.abs(grads["f16x3"][name]["kernel"].astype(np.float64) - grads["f32"][name]["kernel"]).max()
                     / np.abs(grads["f32"][name]["kernel"]).max()) for name, _, _, _ in VGG16}
    ms = median_rounds({bp: (lambda m=m: step(m)) for bp, m in models.items()}, steps, warmup)
    status = models["f16x3"].train_status()
    layers = []
    H = hp["img_size"]
    for i, (name, cin, cout, pool) in enumerate(VGG16):
        f = 2.0 * 9 * cin * cout * B * H * H
        x, dy = torch.randn((B, H, H, cin), device="cuda"), torch.randn((B, H, H, cout), device="cuda")
        dw, db = torch.empty((3, 3, cin, cout), device="cuda"), torch.empty((cout,), device="cuda")
        w = torch.randn((3, 3, cin, cout), device="cuda") * (2.0 / (9 * cin)) ** 0.5
        sizes = [lib.rpn_conv3x3_wgrad_wide_workspace_bytes(B, H, H, cin, cout)]
        if cin % 4 == 0:
            sizes += [lib.rpn_conv3x3_wgrad_wide_x3_workspace_bytes(B, H, H, cin, cout), lib.rpn_conv3x3_dgrad_workspace_bytes(cin, cout),
                      lib.rpn_conv3x3_dgrad_x3_workspace_bytes(cin, cout)]
        ws = torch.empty(max(sizes), dtype=torch.uint8, device="cuda")
        n, s = ws.numel(), L.stream_ptr
        fns = {"ms_wgrad_f32": lambda: L.check(lib.rpn_conv3x3_wgrad_wide(L.ptr(x), L.ptr(dy), B, H, H, cin, cout, L.ptr(dw), L.ptr(db),
                                                                          L.ptr(ws), n, s()), "rpn_conv3x3_wgrad_wide")}
        if cin % 4 == 0:
            dx = torch.empty((B, H, H, cin), device="cuda")
            fns["ms_wgrad_x3"] = lambda: L.check(lib.rpn_conv3x3_wgrad_wide_x3(L.ptr(x), L.ptr(dy), B, H, H, cin, cout, L.ptr(dw), L.ptr(db),
                                                                              None, L.ptr(ws), n, s()), "rpn_conv3x3_wgrad_wide_x3")
            fns["ms_dgrad_f32"] = lambda: L.check(lib.rpn_conv3x3_dgrad(L.ptr(dy), L.ptr(w), L.ptr(x), B, H, H, cin, cout, L.ptr(dx),
                                                                       L.ptr(ws), n, s()), "rpn_conv3x3_dgrad")
            fns["ms_dgrad_x3"] = lambda: L.check(lib.rpn_conv3x3_dgrad_x3(L.ptr(dy), L.ptr(w), L.ptr(x), None, B, H, H, cin, cout, L.ptr(dx),
                                                                         None, L.ptr(ws), n, s()), "rpn_conv3x3_dgrad_x3")
        t = median_rounds(fns, max(2, steps // 2), 1)
        row = {"layer": name, "H": H, "cin": cin, "cout": cout, "gflop": round(f / 1e9, 2), "d": float("%.3e" % d[name])}
        row.update({k: round(v, 4) for k, v in t.items()})
        for kind in ("wgrad", "dgrad"):
            if "ms_%s_x3" % kind in t:
                row["%s_x3_tflops" % kind] = round(f / t["ms_%s_x3" % kind] / 1e9, 1)
                row["%s_speedup" % kind] = round(t["ms_%s_f32" % kind] / t["ms_%s_x3" % kind], 2)
        layers.append(row)
        del x, dy, w, ws
        if pool:
            H //= 2
    return {"backbone": "vgg16", "train_backbone": True, "precision": precision, "batch": B, "ms_train_step_f32": round(ms["f32"], 3),
            "ms_train_step_f16x3": round(ms["f16x3"], 3), "step_speedup": round(ms["f32"] / ms["f16x3"], 3),
            "f16_range": status["f16_range"], "layers": layers}


def bench_mobilenet_span(train_from, precision, B, steps, warmup, feature_grad=False):
    """MobileNetV2 from `train_from` (block_7_expand .. block_13_expand): ms per training / evaluation step, and each new kernel family's
    single-layer entry on the block_12 shape (96 -> 576 -> 96 at F x F) with its fraction of its own floor: bytes / 8 TB/s for the
    BatchNorm and depthwise kernels, the float32-MFMA peak for the two GEMMs."""
    hp = train_utils.get_hyper_params("mobilenet_v2")
    model, _ = rpn_mobilenet_v2.get_model(hp, precision=precision, max_batch=B)
    imgs, deltas, lab = step_inputs(model, hp, B)
    model.compile(learning_rate=1e-5, train_backbone_from=train_from)
    ms_train, ms_eval = step_times(model, imgs, deltas, lab, B, steps, warmup)
    joint = feature_grad_times(model, imgs, deltas, lab, B, steps, warmup) if feature_grad else {}
    lib = L.lib()
    F = model.feature_map_shape
    P, C, Cs = B * F * F, 576, 96
    x, dy = torch.randn((P, C), device="cuda"), torch.randn((P, C), device="cuda")
    y, dx = torch.empty_like(x), torch.empty_like(x)
    xs, dxs = torch.randn((P, Cs), device="cuda"), torch.empty((P, Cs), device="cuda")
    g, b = torch.rand(C, device="cuda") + 0.5, torch.rand(C, device="cuda")
    mean, var, dg, db = (torch.empty(C, device="cuda") for _ in range(4))
    w, dw = torch.randn((Cs, C), device="cuda"), torch.empty((Cs, C), device="cuda")
    wd, dwd = torch.randn((3, 3, C), device="cuda"), torch.empty((3, 3, C), device="cuda")
    nb = lib.rpn_batchnorm_workspace_bytes(P, C)
    nw = lib.rpn_conv1x1_wgrad_workspace_bytes(P, Cs, C)
    nd = lib.rpn_dwconv3x3_wgrad_workspace_bytes(B, F, F, C)
    ws = torch.empty(max(nb, nw, nd, 4), dtype=torch.uint8, device="cuda")
    s = L.stream_ptr
    calls = {
        "batchnorm_train_forward": (lambda: lib.rpn_batchnorm_train_forward(L.ptr(x), P, C, L.ptr(g), L.ptr(b), 1, 1e-3, 0.999, L.ptr(y),
                                                                            L.ptr(mean), L.ptr(var), None, None, L.ptr(ws), nb, s()),
                                    ("bytes", 3.0 * P * C * 4)),          # x read twice (statistics, apply), y written
        "batchnorm_train_backward": (lambda: lib.rpn_batchnorm_train_backward(L.ptr(x), L.ptr(dy), P, C, L.ptr(g), L.ptr(b), L.ptr(mean),
                                                                              L.ptr(var), 1, 1e-3, L.ptr(dx), L.ptr(dg), L.ptr(db),
                                                                              L.ptr(ws), nb, s()),
                                     ("bytes", 5.0 * P * C * 4)),         # x, dy read twice, dx written
        "conv1x1_wgrad": (lambda: lib.rpn_conv1x1_wgrad(L.ptr(xs), L.ptr(dy), P, Cs, C, L.ptr(dw), L.ptr(ws), nw, s()),
                          ("flop", 2.0 * P * Cs * C)),
        "conv1x1_dgrad": (lambda: lib.rpn_conv1x1_dgrad(L.ptr(dy), L.ptr(w), L.ptr(xs), P, Cs, C, L.ptr(dxs), s()), ("flop", 2.0 * P * Cs * C)),
        "dwconv3x3_dgrad": (lambda: lib.rpn_dwconv3x3_dgrad(L.ptr(dy), L.ptr(wd), B, F, F, C, L.ptr(dx), s()), ("bytes", 2.0 * P * C * 4)),
        "dwconv3x3_wgrad": (lambda: lib.rpn_dwconv3x3_wgrad(L.ptr(x), L.ptr(dy), B, F, F, C, L.ptr(dwd), L.ptr(ws), nd, s()),
                            ("bytes", 2.0 * P * C * 4)),
    }
    kernels = {}
    for name, (fn, (kind, amount)) in calls.items():
        def run(fn=fn, name=name):
            L.check(fn(), name)
        ms = timed(run, steps, warmup)
        floor_ms = amount / (8e12 if kind == "bytes" else PEAK_F32_MFMA) * 1e3
        kernels[name] = {"ms": round(ms, 4), "floor_ms": round(floor_ms, 5), "frac_of_floor": round(floor_ms / ms, 3)}
    return dict({"backbone": "mobilenet_v2", "train_backbone_from": train_from, "precision": precision, "batch": B,
                 "ms_train_step": round(ms_train, 3), "ms_eval_step": round(ms_eval, 3), "block_12_shape": [P, Cs, C], "kernels": kernels},
                **joint)


def bench_mobilenet_full(precision, B, steps, warmup, feature_grad=False):
    hp = train_utils.get_hyper_params("mobilenet_v2")
    model, _ = rpn_mobilenet_v2.get_model(hp, precision=precision, max_batch=B)
    imgs, deltas, lab = step_inputs(model, hp, B)
    model.compile(learning_rate=1e-5, train_backbone=True)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    ms_train, ms_eval = step_times(model, imgs, deltas, lab, B, steps, warmup)
    trainer_bytes = free0 - torch.cuda.mem_get_info()[0]               # the trainer allocates at its first step
    joint = feature_grad_times(model, imgs, deltas, lab, B, steps, warmup) if feature_grad else {}
    lib = L.lib()
    s = L.stream_ptr
    img = hp["img_size"]
    H1 = (img + img % 2 + 1 - 3) // 2 + 1                               # Conv1's output side = block_1_depthwise's input side
    H2 = (H1 + H1 % 2 + 1 - 3) // 2 + 1
    C = 96
    x, dy = torch.randn((B, H1, H1, C), device="cuda"), torch.randn((B, H2, H2, C), device="cuda")
    dx, wd, dwd = torch.empty_like(x), torch.randn((3, 3, C), device="cuda"), torch.empty((3, 3, C), device="cuda")
    xi, dys, dws = imgs, torch.randn((B, H1, H1, 32), device="cuda"), torch.empty((3, 3, 3, 32), device="cuda")
    nd = lib.rpn_dwconv3x3_s2_wgrad_workspace_bytes(B, H1, H1, C)
    ns = lib.rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(B, img, img, 32)
    ws = torch.empty(max(nd, ns), dtype=torch.uint8, device="cuda")
    calls = {
        "dwconv3x3_s2_dgrad": (lambda: lib.rpn_dwconv3x3_s2_dgrad(L.ptr(dy), L.ptr(wd), B, H1, H1, C, L.ptr(dx), s()),
                               4.0 * (dy.numel() + dx.numel())),            # dy read, dx written
        "dwconv3x3_s2_wgrad": (lambda: lib.rpn_dwconv3x3_s2_wgrad(L.ptr(x), L.ptr(dy), B, H1, H1, C, L.ptr(dwd), L.ptr(ws), nd, s()),
                               4.0 * (x.numel() + dy.numel())),             # x, dy read
        "conv3x3_s2_cin3_wgrad": (lambda: lib.rpn_conv3x3_s2_cin3_wgrad(L.ptr(xi), L.ptr(dys), B, img, img, 32, L.ptr(dws), L.ptr(ws), ns, s()),
                                  4.0 * (xi.numel() + dys.numel())),        # the images, dy read
    }
    kernels = {}
    for name, (fn, nbytes) in calls.items():
        def run(fn=fn, name=name):
            L.check(fn(), name)
        ms = timed(run, steps, warmup)
        kernels[name] = {"ms": round(ms, 4), "mbytes": round(nbytes / 1e6, 1), "tb_per_s": round(nbytes / ms / 1e9, 3)}
    return dict({"backbone": "mobilenet_v2", "train_backbone": True, "precision": precision, "batch": B, "ms_train_step": round(ms_train, 3),
                 "ms_eval_step": round(ms_eval, 3), "trainer_device_gb": round(trainer_bytes / 1e9, 3), "kernels": kernels}, **joint)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--train-backbone-from", default=None,
                    help="a VGG16 conv, or with --backbone mobilenet_v2 block_7_expand .. block_13_expand: time the trainer that trains it "
                         "and the layers above")
    ap.add_argument("--backbone", default=None, choices=("vgg16", "mobilenet_v2"),
                    help="with --train-backbone-from: the backbone (default vgg16); without: time that backbone's head-only step alone")
    ap.add_argument("--train-backbone", action="store_true",
                    help="time the trainer of compile(train_backbone=True): every layer of --backbone (default vgg16) trains")
    ap.add_argument("--feature-grad", action="store_true",
                    help="with --train-backbone / --train-backbone-from: also time the step in two halves with a second-stage gradient at "
                         "the feature tap (forward_for_training + apply_gradients(G))")
    ap.add_argument("--backward-precision", default=None, choices=("f16x3",),
                    help="VGG16, the whole model: time the float32 and the f16x3 backward step side by side, and the single-layer entries")
    args = ap.parse_args()
    if args.feature_grad and not (args.train_backbone or args.train_backbone_from):
        ap.error("--feature-grad needs a trained backbone span: --train-backbone or --train-backbone-from")
    L.require_gpu()
    fg = args.feature_grad
    if args.backward_precision:
        if args.backbone == "mobilenet_v2" or args.train_backbone_from or fg:
            ap.error("--backward-precision times the whole VGG16 model's step: no --backbone mobilenet_v2, --train-backbone-from, --feature-grad")
        print(json.dumps(bench_backward_x3(args.precision, args.batch, args.steps, args.warmup)), flush=True)
        return
    if args.train_backbone:
        if args.train_backbone_from:
            ap.error("--train-backbone trains every layer: it cannot be combined with --train-backbone-from")
        if args.backbone == "mobilenet_v2":
            print(json.dumps(bench_mobilenet_full(args.precision, args.batch, args.steps, args.warmup, fg)), flush=True)
        else:
            print(json.dumps(bench_backbone("block1_conv1", args.precision, args.batch, args.steps, args.warmup, fg)), flush=True)
        return
    if args.train_backbone_from and args.backbone == "mobilenet_v2":
        print(json.dumps(bench_mobilenet_span(args.train_backbone_from, args.precision, args.batch, args.steps, args.warmup, fg)), flush=True)
        return
    if args.backbone and not args.train_backbone_from:
        print(json.dumps(bench(args.backbone, args.precision, args.batch, args.steps, args.warmup)), flush=True)
        return
    if args.train_backbone_from:
        print(json.dumps(bench_backbone(args.train_backbone_from, args.precision, args.batch, args.steps, args.warmup, fg)), flush=True)
        return
    for backbone in ("vgg16", "mobilenet_v2"):
        print(json.dumps(bench(backbone, args.precision, args.batch, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
