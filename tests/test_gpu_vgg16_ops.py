"""The VGG16 split-precision forward (vgg_block1, conv3x3_split, conv3x3_split16 register-staged and LDS-DMA, maxpool_split, the
K-tree rpn_conv and the head behind it), one op at a time and in every launch form.

Method (tests/vgg_ops.py has the cases, the reference, the emulation and the bounds).  rpn_model_forward_to reads the library's OWN
input of an op (the tensor written by the op before it, or the images) and its output, from one handle and the same images; the op
alone is evaluated in float64 on that input, so an error cannot hide behind the layers above it or be averaged away below it.  Every
op and batch size asserts the launch form it runs from rpn_model_conv_launch_info (kernel family, tile width, pool in the epilogue,
K form) against the case table -- never from ops(), which names the kernel of max_batch.

Per case (precision, img, max_batch) and batch size B of its table:
  * every forward_to and the forward run twice: same bits;
  * the largest batch is compared with float64 on images 0, 1, B / 2 and B - 1, op by op, against both bounds (x3_bound elementwise
    and x3_f32_bound; float32 ops: f32_bound), after the conditions on the inputs are asserted on that reference; rpn_conv where
    forward_to can read it (no split over workgroups at that B), the head pair (reg, cls) from predict_on_batch always;
  * every other image is covered by bit equality on the one handle, the batch invariance include/rpn_hip.h promises -- across the
    form boundaries: the same images at every other batch size of the table, images 0 and B - 1 alone, and the batch REVERSED;
  * nothing left unwritten: forward_to copies the tensor out of the handle's arena into a fresh tensor, and the arena cannot be
    filled with NaN from here.  Instead the first forward of every op runs on the REVERSED batch: a tile a kernel then leaves
    unwritten keeps ANOTHER image's value, finite and plausible, and fails the float64 comparison (the compared images) or the bit
    equality with the reversed batch (all of them).  Finiteness is asserted on every tensor;
  * the keep_activations case: conv without a pool epilogue, then maxpool_split (exact: bound 0) -- and every tensor the fused
    handle writes equals it bit for bit;
  * status()["f16_range"] is false at the end.

Measured on an MI355X (largest over the cases; every case prints each op).  err = largest error against float64,
then x3_f32_bound at that op and the largest share of it over the family's ops, then the largest share of x3_bound:
  vgg_block1 (f16x3)                          2.6e-6   9.4e-6 (0.27)   8.2e-4
  conv3x3_split16 register-staged, 64 wide    1.4e-5   1.8e-5 (0.85)   8.1e-4
  conv3x3_split16 LDS-DMA 64 wide             1.9e-5   2.5e-5 (0.87)   1.6e-4     with the pool epilogue  1.5e-5  1.7e-5 (0.87)  4.3e-4
  conv3x3_split16 LDS-DMA 128 wide            1.5e-5   1.9e-5 (0.83)   1.1e-3     with the pool epilogue  1.4e-5  2.1e-5 (0.80)  4.5e-4
  rpn_conv, the K tree in one workgroup       6.2e-6   2.0e-5 (0.31)   5.1e-5
  head pair (f16x3)                           reg 5.0e-7 under 3.1e-6 (1.5e-6 of its elementwise bound), cls 9.5e-7 under 4.2e-6
  first layer on the MFMA (f16x3, kept)       6.0e-7   7.2e-6 (0.08)   0.017
  conv3x3_split (f16x3, kept)                 2.4e-6   8.2e-6 (0.29)   1.0e-3
  bf16x3: float32 first layer 1.6e-5 under its float32 bound 6.7e-5; conv3x3_split + pool 2.7e-5, 1.1e-4 (0.24), 9.1e-3;
          conv3x3_split16 7.4e-5, 3.0e-4 (0.30), 7.8e-3; head reg 3.3e-6 under 1.4e-5, cls 5.6e-6 under 2.4e-5
  maxpool_split: 0.  The bf16x3 handle that keeps every activation equals the fused one bit for bit on every tensor; under f16x3
  block 1 differs (vgg_block1 against its two separate kernels), so that case holds the float64 bounds only.
The float16 layers with K = 2304 and 4608 use up to 0.87 of x3_f32_bound: the kernels walk K as one float32 chain per leaf, the
CPU emulation's convolution adds in blocks.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vgg_ops as vo  # noqa: E402

pytestmark = pytest.mark.gpu


def _images(case, B):
    top = max(c["max_batch"] for c in vo.CASES if c["img"] == case["img"])
    return vo.images(top, case["img"])[:B].cuda()


def readable(model, name, B):
    """forward_to refuses rpn_conv where the head adds its split-K slabs"""
    return name != "rpn_conv" or vo.form(model, name, B)[3] in (0, 1)


def run_ops(model, case, x, twice=True):
    """{tensor: the op's output for the images x} from one rpn_model_forward_to each, + "reg", "cls" from a forward"""
    B, outs = int(x.shape[0]), {}
    for op in vo.graph(case["precision"], case["keep"]):
        if not readable(model, op["name"], B):
            continue
        outs[op["name"]] = model.forward_to(op["name"], x)
        if twice:
            assert torch.equal(outs[op["name"]], model.forward_to(op["name"], x)), ("run to run", op["name"], B)
    reg, cls = model.predict_on_batch(x)
    outs["reg"], outs["cls"] = reg.clone(), cls.clone()
    if twice:
        reg2, cls2 = model.predict_on_batch(x)
        assert torch.equal(reg2, outs["reg"]) and torch.equal(cls2, outs["cls"]), ("run to run, head", B)
    for name, t in outs.items():
        assert torch.isfinite(t).all().item(), (name, B)
    return outs


def assert_forms(model, case, B):
    for op in vo.graph(case["precision"], case["keep"]):
        assert vo.form(model, op["name"], B) == vo.expected_form(case, op["name"], B), (case["id"], op["name"], B)


def assert_same(a, b, what):
    assert set(a) >= set(b) or set(b) >= set(a)
    for name in set(a) & set(b):
        assert torch.equal(a[name], b[name]), what + (name,)


def check_op(model, op, x_in, got, w, label, B):
    """`got` for the NHWC float32 input x_in (numpy), rows of a forward of B images, against the op alone in float64 -> (error, scalar bound, largest share of the
    elementwise bound)"""
    fmt = model.precision
    ref = vo.op_ref(op, x_in, w)
    vo.input_conditions(ref["out"], "%s %s" % (label, op["name"]))
    err = np.abs(got.astype(np.float64) - ref["out"])
    route = vo.form(model, op["name"], B)[:2]
    if not op["convs"]:
        print("vgg16 ops %s %s %s: err %.3g (a max-pool of exact values: bound 0)" % (label, op["name"], route, err.max()))
        assert err.max() == 0.0, (label, op["name"])
        return 0.0, 0.0, 0.0
    if vo.is_f32_op(model, op):
        bound = vo.f32_bound(ref["out"], vo.op_ref32(op, x_in, w, fmt))
        print("vgg16 ops %s %s %s: err %.3g, float32 bound %.3g" % (label, op["name"], route, err.max(), bound))
        assert err.max() <= bound, (label, op["name"], err.max(), bound)
        return err.max(), bound, err.max() / bound
    elementwise, scalar = vo.x3_bound(op, x_in, ref, w, fmt), vo.x3_f32_bound(op, x_in, ref, w, fmt)
    share = (err / elementwise).max()
    print("vgg16 ops %s %s %s: err %.3g; x3_f32_bound %.3g; x3_bound there %.3g, largest share %.3g"
          % (label, op["name"], route, err.max(), scalar, elementwise.flat[err.argmax()], share))
    assert (err <= elementwise).all(), (label, op["name"], route, share)
    assert err.max() <= scalar, (label, op["name"], route, err.max(), scalar)
    return err.max(), scalar, share


def check_head(model, tap, reg, cls, w, label, B):
    fmt = model.precision
    ref = vo.head_ref(tap, w)
    assert ref["cls"].max() <= 1 - 2.0 ** -22 and ref["cls"].min() >= 2.0 ** -100          # float32 holds such a sigmoid inside (0, 1)
    e_reg, e_cls = vo.emulate_head(tap, w, fmt)
    b_reg, b_cls = vo.scalar_bound(e_reg, ref["reg"]), vo.scalar_bound(e_cls, ref["cls"])
    err_r = np.abs(reg.astype(np.float64).reshape(ref["reg"].shape) - ref["reg"])
    err_c = np.abs(cls.astype(np.float64).reshape(ref["cls"].shape) - ref["cls"])
    elementwise = vo.head_bounds(tap, ref, w, fmt)
    print("vgg16 ops %s head %s: reg err %.3g (scalar bound %.3g, largest share of the elementwise bound %.3g), cls err %.3g (bound %.3g)"
          % (label, model.head_launch_info(B), err_r.max(), b_reg, (err_r / elementwise).max(), err_c.max(), b_cls))
    assert (err_r <= elementwise).all() and err_r.max() <= b_reg and err_c.max() <= b_cls, (label, err_r.max(), b_reg, err_c.max(), b_cls)


@pytest.mark.parametrize("case", vo.CASES, ids=vo.case_ids())
def test_ops(case):
    w = vo.weights()
    model = vo.make(case)
    graph = vo.graph(case["precision"], case["keep"])
    batches = sorted(case["forms"])
    top = batches[-1]
    x = _images(case, top)
    for B in batches:
        assert_forms(model, case, B)
    # (module docstring: the arena first holds the reversed batch)
    rev = run_ops(model, case, x.flip(0).contiguous(), twice=False) if top > 1 else None
    full = run_ops(model, case, x)
    if rev is not None:
        assert_same({k: v.flip(0) for k, v in rev.items()}, full, (case["id"], "reversed batch"))
    rows = sorted({0, min(1, top - 1), top // 2, top - 1})
    compare = [op["name"] for op in graph] + ["head"] if case["compare"] is None else list(case["compare"])
    label = "%s B=%d" % (case["id"], top)
    worst = (0.0, "")
    for op in graph:
        if op["name"] not in compare or op["name"] not in full:
            continue
        x_in = (x if op["src"] == "input" else full[op["src"]])[rows].cpu().numpy()
        res = check_op(model, op, x_in, full[op["name"]][rows].cpu().numpy(), w, label, top)
        worst = max(worst, (res[2], op["name"]))
    if "head" in compare:
        check_head(model, full["block5_conv3"][rows].cpu().numpy(), full["reg"][rows].cpu().numpy(), full["cls"][rows].cpu().numpy(), w, label, top)
    print("vgg16 ops %s: largest share of the elementwise bound %.3g (%s)" % ((case["id"],) + worst))
    # every image, bit for bit: the other batch sizes of the table, two images alone
    for B in batches[:-1]:
        assert_same(run_ops(model, case, x[:B].contiguous()), {k: v[:B] for k, v in full.items()}, (case["id"], "batch", B))
    for i in sorted({0, top - 1}):
        assert_same(run_ops(model, case, x[i:i + 1].contiguous(), twice=False), {k: v[i:i + 1] for k, v in full.items()},
                    (case["id"], "image", i, "alone"))
    assert not model.status()["f16_range"]
    if case["keep"]:
        # the production graph's fused ops write the same bits as conv, then maxpool_split
        fused = vo.make(dict(case, keep=False))
        assert any(vo.form(fused, op["name"], top)[2] for op in vo.graph(case["precision"]))
        got = run_ops(fused, dict(case, keep=False), x, twice=False)
        print("vgg16 ops %s: fused == unfused bit for bit on %s" % (case["id"], sorted(k for k in got if torch.equal(got[k], full[k]))))
        if case["precision"] == "bf16x3":
            assert_same(got, full, (case["id"], "fused against unfused"))
        assert not fused.status()["f16_range"]


# (writer, img, max_batch, producing layer, tensor it writes, expected (family, width, pool), consumer layer, consumer's tensor)
RANGE = [("reg", 96, 2, "block2_conv1", "block2_conv1", ("split16_reg", 64, False), "block2_conv2", "block2_pool"),
         ("dma-pool", 96, 2, "block2_conv2", "block2_pool", ("split16_dma", 64, True), "block3_conv1", "block3_conv1"),
         ("dma", 96, 17, "block2_conv1", "block2_conv1", ("split16_dma", 64, False), "block2_conv2", "block2_pool")]


@pytest.mark.parametrize("writer,img,max_batch,layer,tensor,expected,consumer,consumed", RANGE, ids=[r[0] for r in RANGE])
def test_f16_range_flag(writer, img, max_batch, layer, tensor, expected, consumer, consumed):
    """The SPLIT16 writers of conv3x3_split16 (register-staged; LDS-DMA without and with the pool epilogue) raise
    RPN_STATUS_F16_RANGE when a value they write leaves the float16 range: the producing layer's kernel and bias times 2^14 and the
    consumer's kernel times 2^-14 change only the producer's output (ReLU is positively homogeneous), which then passes 65504."""
    base = vo.weights()
    case = dict(precision="f16x3", img=img, max_batch=max_batch, keep=False)
    x = vo.images(17, img)[:max_batch].cuda()
    model = vo.make(case)
    assert vo.form(model, tensor, max_batch)[:3] == expected
    produced = model.forward_to(tensor, x)
    assert float(produced.max()) * 2.0 ** 14 > 65504.0 and not model.status()["f16_range"]
    want = model.forward_to(consumed, x)
    model.set_weights(vo.scaled_layer(base, layer, consumer, 14))
    model.forward_to(tensor, x)
    assert model.status(reset=True)["f16_range"]              # raised by the writer itself
    assert not model.status()["f16_range"]
    model.set_weights(base)
    assert torch.equal(model.forward_to(consumed, x), want)
    assert not model.status()["f16_range"]
