"""Per-layer dgrad / wgrad times of the VGG16 backbone training step, per dispatch, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- \\
        python scripts/train_step_bench.py --train-backbone-from block1_conv1 --steps 10 --warmup 2
    python scripts/train_backbone_trace.py OUT/run_kernel_trace.csv --train-backbone-from block1_conv1

A training step ends with its one adam_kernel dispatch.  Between the previous step's adam_kernel (or the start of the trace) and
this one, the backward's dispatches come in a fixed order (trainer.hip, backbone_backward): conv3x3_dgrad_f32_kernel for
rpn_conv's input first, then for conv i = 12 .. first trained: conv3x3_wgrad_f32_kernel<true> (the instance with the row of ones
behind db; the head's rpn_conv runs <false>) (+ wgrad_tree_kernel levels + wgrad_wide_finish_kernel), then, above the first trained conv, conv3x3_dgrad_f32_kernel (+ maxpool2x2_backward_kernel where a pool
sits below).  Each dispatch is attributed to its layer by that order; the evaluation steps and single-layer timings the bench runs
afterwards follow the last adam_kernel and are not counted.  Prints one line per layer: mean us per step of each kernel, with the
dgrad / wgrad GEMM rate against the 157.3 TF/s float32-MFMA peak at the bench's batch and 500 x 500.
"""
import argparse
import csv

PEAK_F32_MFMA = 157.3e12
VGG16 = [("block1_conv1", 3, 64, False), ("block1_conv2", 64, 64, True), ("block2_conv1", 64, 128, False),
         ("block2_conv2", 128, 128, True), ("block3_conv1", 128, 256, False), ("block3_conv2", 256, 256, False),
         ("block3_conv3", 256, 256, True), ("block4_conv1", 256, 512, False), ("block4_conv2", 512, 512, False),
         ("block4_conv3", 512, 512, True), ("block5_conv1", 512, 512, False), ("block5_conv2", 512, 512, False),
         ("block5_conv3", 512, 512, False)]


def kind(name):
    for k in ("conv3x3_dgrad_f32_kernel", "conv3x3_wgrad_f32_kernel<true>", "wgrad_tree_kernel", "wgrad_wide_finish_kernel",
              "maxpool2x2_backward_kernel", "dgrad_weights_kernel", "adam_kernel"):
        if k in name:
            return k
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--train-backbone-from", default="block1_conv1")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--img", type=int, default=500)
    args = ap.parse_args()
    rows = sorted(csv.DictReader(open(args.trace)), key=lambda r: int(r["Start_Timestamp"]))
    first = [v[0] for v in VGG16].index(args.train_backbone_from)
    steps, cur = [], []
    for r in rows:
        k = kind(r["Kernel_Name"])
        if k is None:
            continue
        if k == "adam_kernel":
            steps.append(cur)
            cur = []
        else:
            cur.append((k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    acc = {}
    for disp in steps:
        # the GEMM dispatches in order: dgrad for rpn_conv, then wgrad of conv 12, dgrad of conv 12, ..., wgrad of the first trained
        # conv; the smaller kernels after a GEMM (leaf tree, finish, the next weight flip, max-pool backward) go to that GEMM's layer
        n_w = n_d = 0
        layer = None
        for k, us in disp:
            if k == "conv3x3_dgrad_f32_kernel":
                layer, what = ("rpn_conv" if n_d == 0 else VGG16[13 - n_d][0]), "dgrad"
                n_d += 1
            elif k == "conv3x3_wgrad_f32_kernel<true>":
                layer, what = VGG16[12 - n_w][0], "wgrad"
                n_w += 1
            elif layer is None:
                continue
            else:
                what = "other"
            acc.setdefault(layer, {}).setdefault(what, {}).setdefault(id(disp), 0.0)
            acc[layer][what][id(disp)] += us
        assert n_w == 13 - first and n_d == 13 - first, (n_w, n_d)
    mean = lambda d: sum(d.values()) / len(d) if d else float("nan")
    frac = lambda f, us: f / (us * 1e-6) / PEAK_F32_MFMA if us == us else float("nan")
    print("%d training steps (mean us per step)" % len(steps))
    print("%-13s %5s %11s %10s %7s %10s %7s %10s" % ("layer", "side", "cin->cout", "wgrad", "/peak", "dgrad", "/peak", "other"))
    H = args.img
    for name, cin, cout, pool in VGG16:
        f = 2.0 * 9 * cin * cout * args.batch * H * H
        d = acc.get(name, {})
        w_us, d_us = mean(d.get("wgrad", {})), mean(d.get("dgrad", {}))
        print("%-13s %5d %5d->%-5d %10.1f %7.3f %10.1f %7.3f %10.1f" % (name, H, cin, cout, w_us, frac(f, w_us), d_us, frac(f, d_us),
                                                                        mean(d.get("other", {}))))
        if pool:
            H //= 2


if __name__ == "__main__":
    main()
