"""The fused MobileNetV2 forward blocks (tf_rpn_amd/csrc/mnv2_block_kernels.hip), one block at a time.

Method (tests/mnv2_blocks.py has the cases, the reference and the bounds).  rpn_model_forward_to reads the library's OWN input of
block k (the output of block k - 1, or the images) and its output, from one handle and the same images; block k is evaluated in
float64 on that input, so an error cannot hide behind the twelve blocks above it.  Every block and batch size asserts the launch form
it ran from rpn_model_ir_launch_info (kernel family, chunk size, K-split factor, tiles) against the case table.

Per case (precision, img, max_batch) and batch size B of its table:
  * every forward_to runs twice: same bits (the K-split tickets are back at zero, no stale partial is read);
  * the largest batch is compared with float64 on images 0, 1, B / 2 and B - 1 (a tile belongs to one image, the partial buffers
    are indexed by tile), after the conditions on the inputs (mnv2_blocks.input_conditions) are asserted on that reference;
  * every image is covered by bit equality on the one handle, the contract of include/rpn_hip.h: the same images at every other
    batch size of the table, images 0 and B - 1 alone at B = 1, and the whole batch in REVERSED order (every image on other tiles,
    other partial-buffer slots) must give the bits of the largest batch.  What equals a row that lies inside the bound lies inside it.

Bounds: float32 routes 4 d32 + 1e-6 max(1, max|ref64|); f16x3 routes the a-priori elementwise x3_bound AND the scalar x3_f32_bound
(mnv2_blocks.py).  Measured on an MI355X, largest over the cases (every case prints its own figures):
  f32     9.5e-6 under a bound of 4.0e-5 (block 12 at img 150; outputs up to 21)
  bf16x3  7.7e-6 under 3.8e-5, and the f32 handle's bits on every block
  f16x3   the f16x3 kernels 4.5e-6 under x3_f32_bound = 2.8e-5 (largest share 0.17) and 9.4e-4 of x3_bound; its float32 stem 3.6e-6
          under 2.5e-5
The float32 block 3 (ir_block below 512 tiles, ir_block_hr from 512 on) gives the same bits at 8, 504 and 512 tiles.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mnv2_blocks as mb  # noqa: E402

pytestmark = pytest.mark.gpu


def run_blocks(model, x, twice=True):
    """[output of block k for the images x], k = 0 .. 12, each from its own rpn_model_forward_to"""
    outs = []
    for k in range(mb.NBLOCKS):
        out = model.forward_to(mb.tensor_name(k), x)
        if twice:
            assert torch.equal(out, model.forward_to(mb.tensor_name(k), x)), ("run to run", k, int(x.shape[0]))
        outs.append(out)
    return outs


def assert_forms(model, case, B):
    for k in range(mb.NBLOCKS):
        assert mb.form(model, k, B) == mb.expected_form(case, k, B), (case["id"], k, B)


def check_block(model, k, x_in, got, w, label, conditions=True):
    """block k's output `got` for the NHWC float32 input x_in (numpy) against float64 -> (error, bound, share of the bound)"""
    ref = mb.block_ref(k, x_in, w, torch.float64)
    if conditions:
        mb.input_conditions(k, ref, w, label)
    assert np.isfinite(got).all(), (label, k)
    err = np.abs(got.astype(np.float64) - ref["out"])
    route = model.ir_launch_info(mb.tensor_name(k), 1)["route"]
    if route in mb.F32_ROUTES:
        bound = mb.f32_bound(ref["out"], mb.block_ref(k, x_in, w, torch.float32)["out"])
        print("mnv2 %s block %d %s: err %.3g, float32 bound %.3g" % (label, k, route, err.max(), bound))
        assert err.max() <= bound, (label, k, route, err.max(), bound)
        return err.max(), bound, err.max() / bound
    elementwise, scalar = mb.x3_bound(k, ref, w), mb.x3_f32_bound(k, x_in, ref, w)
    share = (err / elementwise).max()
    print("mnv2 %s block %d %s: err %.3g; x3_f32_bound %.3g; x3_bound there %.3g, largest share %.3g"
          % (label, k, route, err.max(), scalar, elementwise.flat[err.argmax()], share))
    assert (err <= elementwise).all(), (label, k, route, share)
    assert err.max() <= scalar, (label, k, route, err.max(), scalar)
    return err.max(), scalar, err.max() / scalar


@pytest.mark.parametrize("case", mb.CASES, ids=mb.case_ids())
def test_blocks(case):
    w = mb.weights()
    model = mb.make(case["precision"], case["img"], case["max_batch"])
    batches = sorted(case["forms"])
    top = batches[-1]
    x = mb.images(max(c["max_batch"] for c in mb.CASES if c["img"] == case["img"]), case["img"])[:top].cuda()
    assert_forms(model, case, top)
    full = run_blocks(model, x)
    rows = sorted({0, min(1, top - 1), top // 2, top - 1})
    worst = (0.0, 0.0, 0.0, -1)
    for k in range(mb.NBLOCKS):
        x_in = (x if k == 0 else full[k - 1])[rows].cpu().numpy()
        got = full[k][rows].cpu().numpy()
        res = check_block(model, k, x_in, got, w, "%s B=%d" % (case["id"], top))
        worst = max(worst, res[2:] + res[:2] + (k,))
    print("mnv2 %s: largest share of its bound %.3g (err %.3g, bound %.3g, block %d)" % ((case["id"],) + worst))
    # every image, bit for bit: the other batch sizes of the table, two images alone, the batch reversed
    for B in batches[:-1]:
        assert_forms(model, case, B)
        for k, out in enumerate(run_blocks(model, x[:B])):
            assert torch.equal(out, full[k][:B]), (case["id"], "batch", B, "block", k)
    for i in sorted({0, top - 1}):
        for k, out in enumerate(run_blocks(model, x[i:i + 1], twice=False)):
            assert torch.equal(out[0], full[k][i]), (case["id"], "image", i, "alone, block", k)
    if top > 1:
        for k, out in enumerate(run_blocks(model, x.flip(0).contiguous(), twice=False)):
            assert torch.equal(out.flip(0), full[k]), (case["id"], "reversed batch, block", k)
    assert not model.status()["f16_range"]
    if case["precision"] == "bf16x3":
        # bfloat16 splits have no block kernels: the float32 routes, and the float32 handle's bits on every block
        twin = mb.make("f32", case["img"], case["max_batch"])
        for k, out in enumerate(run_blocks(twin, x, twice=False)):
            assert mb.form(twin, k, top) == mb.form(model, k, top) and mb.form(twin, k, top)[0] in mb.F32_ROUTES
            assert torch.equal(out, full[k]), ("bf16x3 against f32, block", k)


# (kernel family, producing projection's BatchNorm, tensor it writes, consumer tensor)
RANGE = [("hrx3", "expanded_conv_project_BN", "expanded_conv_project", "block_1_project"),
         ("x3", "block_6_project_BN", "block_6_project", "block_7_project"),
         ("pw_x3", "block_12_project_BN", "block_12_project", "block_13_expand")]


@pytest.mark.parametrize("family,bn,producer,consumer", RANGE, ids=[r[0] for r in RANGE])
def test_f16_range_flag(family, bn, producer, consumer):
    """Each f16x3 kernel family that splits a float32 input into float16 halves raises RPN_STATUS_F16_RANGE when that input leaves the
    float16 range: the producing projection's BatchNorm gamma and beta times 2^14 put its float32 output beyond 65504."""
    base = mb.weights()
    big = mb.scaled_projection(base, bn)
    x = mb.images(2, 64).cuda()
    model = mb.make("f16x3", 64, 2, big)
    kernels = {op["name"]: op["kernel"] for op in model.ops()}
    assert kernels[consumer].startswith({"hrx3": "ir_block_hr_f16x3<16,", "x3": "ir_block_f16x3<64,", "pw_x3": "pw_f16x3<"}[family])
    model.status(reset=True)
    produced = model.forward_to(producer, x)
    assert float(produced.abs().max()) > 65504.0 and torch.isfinite(produced).all().item()
    assert not model.status()["f16_range"]                       # the producer writes float32: nothing to flag yet
    model.forward_to(consumer, x)
    assert model.status(reset=True)["f16_range"]
    assert not model.status()["f16_range"]
    model.set_weights(base)
    model.forward_to(consumer, x)
    assert not model.status()["f16_range"]
    # the float32 handle takes the same weights: inside its bound on the consumer, and no flag
    f32 = mb.make("f32", 64, 2, big)
    x_in = f32.forward_to(producer, x).cpu().numpy()
    got = f32.forward_to(consumer, x).cpu().numpy()
    assert np.abs(x_in).max() > 65504.0
    if family == "pw_x3":
        ref64, ref32 = (mb.pointwise_ref(x_in, big, consumer, dt) for dt in (torch.float64, torch.float32))
        err, bound = np.abs(got - ref64).max(), mb.f32_bound(ref64, ref32)
        print("mnv2 range %s: f32 block_13_expand err %.3g, bound %.3g" % (family, err, bound))
        assert err <= bound
    else:
        check_block(f32, int(consumer.split("_")[1]), x_in, got, big, "range %s f32" % family, conditions=False)
    assert not f32.status()["f16_range"]
