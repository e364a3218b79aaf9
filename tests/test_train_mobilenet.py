"""Training of MobileNetV2's stride-16 blocks (block_7 .. block_12, block_13_expand) with BatchNorm in training mode:
``compile(train_backbone_from="block_N_expand")``, the BatchNorm / 1x1 / depthwise backward kernels, and the whole-span step.

Oracles: numpy / torch on the CPU.  Integer-valued inputs make the conv backward kernels exact in float32 whatever the summation
order; real-valued checks compare against torch float64 and are bounded by 4 x the largest deviation torch float32 shows on the same
inputs (relative to max |reference| of each tensor): another, equally valid, summation order may cost that much.

BatchNorm as TF 2.0's fused BatchNorm computes it (restated as recalled -- nothing here can run TF): batch mean and biased batch
variance, eps 1e-3; moving = moving * 0.999 + batch * 0.001 with Bessel's correction on the variance; Relu6Grad is strict on both sides.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402
import cases  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models import _rpn_model as M  # noqa: E402
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, RPNModel, synthetic_weights  # noqa: E402
from tf_rpn_amd.utils import train_utils  # noqa: E402

EPS32 = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))
BN_EPS, BN_MOMENTUM = 1e-3, 0.999
# the update's two constants as float32 arithmetic forms them (1 - 0.999f is 0.00100004673, not 0.001)
MOM32 = float(np.float32(BN_MOMENTUM))
ONE_MINUS_MOM32 = float(np.float32(1.0) - np.float32(BN_MOMENTUM))
TF = torch.nn.functional
SPAN = tuple("block_%d_%s" % (b, p) for b in range(7, 13) for p in ("expand", "depthwise", "project")) + ("block_13_expand",)
NEW_SYMBOLS = ("rpn_head_trainer_set_bn", "rpn_head_trainer_get_bn", "rpn_head_trainer_get_bn_gradient", "rpn_batchnorm_workspace_bytes",
               "rpn_batchnorm_train_forward", "rpn_batchnorm_train_backward", "rpn_conv1x1_wgrad_workspace_bytes", "rpn_conv1x1_wgrad",
               "rpn_conv1x1_dgrad", "rpn_dwconv3x3_dgrad", "rpn_dwconv3x3_wgrad_workspace_bytes", "rpn_dwconv3x3_wgrad")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


def hp_for(img):
    return bo.get_hyper_params("mobilenet_v2", img_size=img, feature_map_shape=(img + 15) // 16)


def seeded_model(hp, B, from_layer, seed=3):
    """A MobileNetV2 model compiled with train_backbone_from, its weights given to the Python side only (no device needed)."""
    m = RPNModel("mobilenet_v2", hp, max_batch=B)
    w = synthetic_weights("mobilenet_v2", hp, seed=seed)
    for name in HEAD_LAYERS:
        m._head[name] = (w[name]["kernel"], w[name]["bias"])
    for name in SPAN:
        m._mn[name] = dict({"kernel": w[name]["kernel"]}, **w[name + "_BN"])
    m.compile(train_backbone_from=from_layer)
    return m, w


# ---- CPU: the Python surface and the ABI ----------------------------------------------------------------------------------
def test_compile_from_block12_returns_the_trained_span(lib):
    assert M.MOBILENET_V2_TRAIN_FROM == tuple("block_%d_expand" % b for b in range(7, 14))
    m, w = seeded_model(hp_for(224), 1, "block_12_expand")
    assert m.trained_layers() == ("block_12_expand", "block_12_depthwise", "block_12_project", "block_13_expand", "rpn_conv", "rpn_cls",
                                  "rpn_reg")
    got = m.get_weights()
    convs = m.trained_layers()[:4]
    assert set(got) == set(m.trained_layers()) | {c + "_BN" for c in convs}
    for name in HEAD_LAYERS:
        assert np.array_equal(got[name]["kernel"], w[name]["kernel"]) and np.array_equal(got[name]["bias"], w[name]["bias"]), name
    for name in convs:
        assert set(got[name]) == {"kernel"} and np.array_equal(got[name]["kernel"], w[name]["kernel"]), name
        assert set(got[name + "_BN"]) == {"gamma", "beta", "mean", "var"}
        for key in ("gamma", "beta", "mean", "var"):
            assert np.array_equal(got[name + "_BN"][key], w[name + "_BN"][key]), (name, key)
    # a layer below the span is frozen: the trainer says so, for its kernel and for its BatchNorm
    k = np.empty((1, 1, 576, 96), np.float32)
    st = lib.rpn_head_trainer_get_gradient(m._t, b"block_11_project", k.ctypes.data_as(L.c_float_p), None, None)
    assert st == L.RPN_ERR_INVALID and b"frozen" in lib.rpn_last_error()
    st = lib.rpn_head_trainer_get_layer(m._t, b"block_6_project", k.ctypes.data_as(L.c_float_p), None, None)
    assert st == L.RPN_ERR_INVALID and b"frozen" in lib.rpn_last_error()
    g = np.empty((96,), np.float32)
    gp = g.ctypes.data_as(L.c_float_p)
    assert lib.rpn_head_trainer_get_bn(m._t, b"block_11_project_BN", gp, gp, gp, gp, None) == L.RPN_ERR_INVALID
    assert b"frozen" in lib.rpn_last_error()
    assert lib.rpn_head_trainer_get_bn_gradient(m._t, b"block_12_project_BN", gp, gp, None) == L.RPN_ERR_INVALID   # no step has run
    # a trained conv has no bias
    k12 = np.empty((1, 1, 96, 576), np.float32)
    assert lib.rpn_head_trainer_set_layer(m._t, b"block_12_expand", k12.ctypes.data_as(L.c_float_p), gp) == L.RPN_ERR_INVALID
    assert b"no bias" in lib.rpn_last_error()
    # compiling again without train_backbone_from returns to the head-only trainer
    m.compile()
    assert m.trained_layers() == HEAD_LAYERS and set(m.get_weights()) == set(HEAD_LAYERS)


def test_save_and_load_round_trip_keys(lib, tmp_path):
    m, w = seeded_model(hp_for(80), 1, "block_13_expand")
    got = m.get_weights()
    assert set(got) == set(HEAD_LAYERS) | {"block_13_expand", "block_13_expand_BN"}
    path = str(tmp_path / "w.npz")
    RPNModel.save_weights(got, path)
    data = np.load(path)
    assert "block_13_expand/kernel" in data.files and "block_13_expand_BN/var" in data.files
    assert np.array_equal(data["block_13_expand_BN/gamma"], w["block_13_expand_BN"]["gamma"])


def test_rejected_names_list_what_is_accepted(lib):
    m = RPNModel("mobilenet_v2", hp_for(80), max_batch=1)
    for name in ("block_6_expand", "Conv1", "block_12_project", "block1_conv1"):
        with pytest.raises(ValueError, match="head only") as e:
            m.compile(train_backbone_from=name)
        assert "block_7_expand" in str(e.value) and "block_13_expand" in str(e.value)
        t = L.vp(0)
        assert lib.rpn_model_trainer_create(m._h, name.encode(), ctypes.byref(t)) == L.RPN_ERR_INVALID
        msg = lib.rpn_last_error()
        assert b"block_7_expand" in msg and b"block_13_expand" in msg and b"head only" in msg
    # a VGG16 handle still refuses MobileNetV2 names
    v = RPNModel("vgg16", bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14), max_batch=1)
    with pytest.raises(ValueError, match="not a VGG16 conv"):
        v.compile(train_backbone_from="block_12_expand")


def test_new_entries_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in L.exported_symbols(), name
        assert hasattr(raw, name), name
    assert lib.rpn_abi_version() == 1


def test_new_entries_validate_before_device_use(lib):
    p = L.vp(64)                                    # never dereferenced: validation comes first
    ws = 1 << 20
    assert lib.rpn_batchnorm_workspace_bytes(75, 384) > 0 and lib.rpn_batchnorm_workspace_bytes(75, 3) == 0
    assert lib.rpn_batchnorm_train_forward(p, 75, 6, p, p, 1, 1e-3, 0.999, p, p, p, None, None, p, ws, None) == L.RPN_ERR_INVALID
    assert b"multiple of 4" in lib.rpn_last_error()
    assert lib.rpn_batchnorm_train_forward(p, 75, 8, p, p, 1, 1e-3, 0.999, p, p, p, p, None, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_batchnorm_train_forward(None, 75, 8, p, p, 1, 1e-3, 0.999, p, p, p, None, None, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_batchnorm_train_forward(p, 75, 8, p, p, 1, 1e-3, 0.999, p, p, p, None, None, p, 16, None) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_batchnorm_train_backward(p, p, 0, 8, p, p, p, p, 1, 1e-3, p, p, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_batchnorm_train_backward(p, p, 75, 8, p, p, p, p, 2, 1e-3, p, p, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv1x1_wgrad(p, p, 75, 64, 30, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv1x1_wgrad(p, p, 8192, 576, 96, p, None, 0, None) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_conv1x1_wgrad_workspace_bytes(75, 64, 384) == 0          # one leaf: no scratch
    assert lib.rpn_conv1x1_dgrad(p, p, None, 75, 62, 96, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv1x1_dgrad(p, None, None, 75, 64, 96, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_dwconv3x3_dgrad(p, p, 1, 5, 5, 6, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_dwconv3x3_wgrad(p, p, 1, 5, 0, 8, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_dwconv3x3_wgrad(p, p, 1, 5, 5, 8, p, None, 0, None) == L.RPN_ERR_WORKSPACE


def test_unknown_layer_is_not_called_frozen_and_pointers_must_be_aligned(lib):
    m, _ = seeded_model(hp_for(80), 1, "block_12_expand")
    k = np.empty((3, 3, 512, 512), np.float32)
    kp = k.ctypes.data_as(L.c_float_p)
    for name in (b"block_12_expnad", b"block1_conv1"):               # a typo, a VGG16 conv: no layer of this model
        assert lib.rpn_head_trainer_get_layer(m._t, name, kp, kp, None) == L.RPN_ERR_INVALID
        msg = lib.rpn_last_error()
        assert b"no layer named" in msg and b"frozen" not in msg, msg
    assert lib.rpn_head_trainer_get_layer(m._t, b"Conv1", kp, None, None) == L.RPN_ERR_INVALID
    assert b"frozen" in lib.rpn_last_error()
    # the single-layer entries read float4: a pointer 4 bytes off is refused before any device use
    p, q, ws = L.vp(64), L.vp(68), 1 << 22
    assert lib.rpn_batchnorm_train_forward(q, 75, 8, p, p, 1, 1e-3, 0.999, p, p, p, None, None, p, ws, None) == L.RPN_ERR_INVALID
    assert b"16-byte aligned" in lib.rpn_last_error()
    assert lib.rpn_batchnorm_train_backward(p, p, 75, 8, q, p, p, p, 1, 1e-3, p, p, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv1x1_wgrad(p, q, 75, 64, 96, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv1x1_dgrad(p, p, q, 75, 64, 96, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_dwconv3x3_dgrad(p, q, 1, 5, 5, 8, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_dwconv3x3_wgrad(p, p, 1, 5, 5, 8, q, p, ws, None) == L.RPN_ERR_INVALID
    assert b"16-byte aligned" in lib.rpn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_new_entries_need_a_device(lib):
    p = L.vp(64)
    ws = 1 << 22
    assert lib.rpn_batchnorm_train_forward(p, 75, 8, p, p, 1, 1e-3, 0.999, p, p, p, None, None, p, ws, None) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()
    assert lib.rpn_batchnorm_train_backward(p, p, 75, 8, p, p, p, p, 1, 1e-3, p, p, p, p, ws, None) == L.RPN_ERR_NO_DEVICE
    assert lib.rpn_conv1x1_wgrad(p, p, 75, 64, 96, p, p, ws, None) == L.RPN_ERR_NO_DEVICE
    assert lib.rpn_conv1x1_dgrad(p, p, None, 75, 64, 96, p, None) == L.RPN_ERR_NO_DEVICE
    assert lib.rpn_dwconv3x3_dgrad(p, p, 1, 5, 5, 8, p, None) == L.RPN_ERR_NO_DEVICE
    assert lib.rpn_dwconv3x3_wgrad(p, p, 1, 5, 5, 8, p, p, ws, None) == L.RPN_ERR_NO_DEVICE


# ---- GPU: single kernels, bit-exact on small integers -----------------------------------------------------------------------
def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ints(rng, shape, lo=-3, hi=4):
    return rng.randint(lo, hi, size=shape).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("P,Cin,Cout", [(75, 64, 384), (75, 576, 96), (392, 96, 576), (40, 96, 96)])
def test_conv1x1_backward_integer_bit_exact(lib, P, Cin, Cout):
    """(40, 96, 96): P below one 64-row tile and channel counts that are no multiple of it."""
    rng = np.random.RandomState(P + Cin)
    x, dy, w, add = ints(rng, (P, Cin)), ints(rng, (P, Cout)), ints(rng, (Cin, Cout)), ints(rng, (P, Cin))
    x_d, dy_d, w_d, add_d = cuda(x), cuda(dy), cuda(w), cuda(add)
    dx_out = torch.full((P, Cin), 7.0, device="cuda")
    dw_out = torch.full((Cin, Cout), 7.0, device="cuda")
    nb = lib.rpn_conv1x1_wgrad_workspace_bytes(P, Cin, Cout)
    assert (nb > 0) == (P >= 128)                                   # 392 pixels run as several leaves, 75 as one
    ws = torch.empty((max(nb, 4),), dtype=torch.uint8, device="cuda")
    L.check(lib.rpn_conv1x1_wgrad(L.ptr(x_d), L.ptr(dy_d), P, Cin, Cout, L.ptr(dw_out), L.ptr(ws), nb, L.stream_ptr()), "wgrad")
    assert np.array_equal(dw_out.cpu().numpy(), (x.astype(np.float64).T @ dy.astype(np.float64)).astype(np.float32))
    ref = dy.astype(np.float64) @ w.astype(np.float64).T
    L.check(lib.rpn_conv1x1_dgrad(L.ptr(dy_d), L.ptr(w_d), None, P, Cin, Cout, L.ptr(dx_out), L.stream_ptr()), "dgrad")
    assert np.array_equal(dx_out.cpu().numpy(), ref.astype(np.float32))
    L.check(lib.rpn_conv1x1_dgrad(L.ptr(dy_d), L.ptr(w_d), L.ptr(add_d), P, Cin, Cout, L.ptr(dx_out), L.stream_ptr()), "dgrad+add")
    assert np.array_equal(dx_out.cpu().numpy(), (ref + add).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,C", [(3, 5, 384), (3, 5, 576), (2, 14, 576), (1, 3, 8)])
def test_depthwise_backward_integer_bit_exact(lib, B, H, C):
    rng = np.random.RandomState(B * H + C)
    x, dy, w = ints(rng, (B, H, H, C)), ints(rng, (B, H, H, C)), ints(rng, (3, 3, C))
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    wt = torch.tensor(w.astype(np.float64), requires_grad=True)
    y = TF.conv2d(xt.permute(0, 3, 1, 2), wt.permute(2, 0, 1).unsqueeze(1), padding=1, groups=C).permute(0, 2, 3, 1)
    y.backward(torch.tensor(dy.astype(np.float64)))
    x_d, dy_d, w_d = cuda(x), cuda(dy), cuda(w)                     # named: a temporary's memory is reused by the next allocation
    dx_out = torch.full((B, H, H, C), 7.0, device="cuda")
    dw_out = torch.full((3, 3, C), 7.0, device="cuda")
    L.check(lib.rpn_dwconv3x3_dgrad(L.ptr(dy_d), L.ptr(w_d), B, H, H, C, L.ptr(dx_out), L.stream_ptr()), "dw dgrad")
    assert np.array_equal(dx_out.cpu().numpy(), xt.grad.numpy().astype(np.float32))
    nb = lib.rpn_dwconv3x3_wgrad_workspace_bytes(B, H, H, C)
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    L.check(lib.rpn_dwconv3x3_wgrad(L.ptr(x_d), L.ptr(dy_d), B, H, H, C, L.ptr(dw_out), L.ptr(ws), nb, L.stream_ptr()), "dw wgrad")
    assert np.array_equal(dw_out.cpu().numpy(), wt.grad.numpy().astype(np.float32))


# ---- GPU: BatchNorm forward / backward on real values -----------------------------------------------------------------------------
def bn_torch(x, gamma, beta, dy, relu6, dtype):
    xt = torch.tensor(x.astype(np.float64)).to(dtype).requires_grad_(True)
    g = torch.tensor(gamma.astype(np.float64)).to(dtype).requires_grad_(True)
    b = torch.tensor(beta.astype(np.float64)).to(dtype).requires_grad_(True)
    y = TF.batch_norm(xt, None, None, g, b, training=True, eps=BN_EPS)
    pre = y
    if relu6:
        y = TF.hardtanh(y, 0.0, 6.0)
    y.backward(torch.tensor(dy.astype(np.float64)).to(dtype))
    mean = xt.detach().mean(0)
    var = xt.detach().var(0, unbiased=False)
    out = {"y": y, "mean": mean, "var": var, "dx": xt.grad, "dgamma": g.grad, "dbeta": b.grad}
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}, pre.detach().to(torch.float64).numpy()


def rel_dev(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("P", [75, 392])
@pytest.mark.parametrize("relu6", [1, 0])
def test_batchnorm_training_forward_backward_against_float64(lib, P, relu6):
    """C = 384; channel 5 has mean 100 and spread 0.1: E[x^2] - mean^2 in float32 loses every digit of that variance.
    Bound: 4 x the largest deviation of torch float32 from torch float64 over the six outputs (relative to max |reference| of each).
    Measured on the MI355X (DESIGN.md 6d has the table): P = 75, relu6 = 1: torch float32 worst 7.6e-6, bound 3.05e-5, this code's
    worst 3.3e-6 (y); P = 392: 1.15e-5, 4.61e-5, 6.8e-6 (y)."""
    C = 384
    for seed in range(20):                  # no ReLU6 input within 1e-4 of 0 or 6 in the float64 run
        rng = np.random.RandomState(100 * P + seed)
        x = rng.standard_normal((P, C)).astype(np.float32)
        x[:, 5] = (100.0 + 0.1 * rng.standard_normal(P)).astype(np.float32)
        x[:, 6] = (-3.0 + 5.0 * rng.standard_normal(P)).astype(np.float32)
        gamma = rng.uniform(0.8, 1.2, C).astype(np.float32)
        beta = rng.uniform(2.7, 3.3, C).astype(np.float32)          # ReLU6 clamps both tails, about 0.1 % each
        dy = rng.standard_normal((P, C)).astype(np.float32)
        ref, pre = bn_torch(x, gamma, beta, dy, relu6, torch.float64)
        if not relu6 or min(np.abs(pre).min(), np.abs(pre - 6.0).min()) > 1e-4:
            break
    else:
        pytest.fail("no seed keeps the ReLU6 inputs away from 0 and 6")
    if relu6:
        assert (pre <= 0).sum() > 0 and (pre >= 6).sum() > 0      # the mask is exercised on both sides
    t32, _ = bn_torch(x, gamma, beta, dy, relu6, torch.float32)
    bound = 4.0 * max(rel_dev(t32[k], ref[k]) for k in ref)
    mm0, mv0 = rng.uniform(-0.1, 0.1, C).astype(np.float32), rng.uniform(0.8, 1.2, C).astype(np.float32)
    d = {k: cuda(v) for k, v in dict(x=x, gamma=gamma, beta=beta, dy=dy, mm=mm0, mv=mv0).items()}
    y, dx = torch.empty((P, C), device="cuda"), torch.empty((P, C), device="cuda")
    mean, var, dg, db = (torch.empty((C,), device="cuda") for _ in range(4))
    nb = lib.rpn_batchnorm_workspace_bytes(P, C)
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    L.check(lib.rpn_batchnorm_train_forward(L.ptr(d["x"]), P, C, L.ptr(d["gamma"]), L.ptr(d["beta"]), relu6, BN_EPS, BN_MOMENTUM, L.ptr(y),
                                            L.ptr(mean), L.ptr(var), L.ptr(d["mm"]), L.ptr(d["mv"]), L.ptr(ws), nb, L.stream_ptr()), "bn fwd")
    L.check(lib.rpn_batchnorm_train_backward(L.ptr(d["x"]), L.ptr(d["dy"]), P, C, L.ptr(d["gamma"]), L.ptr(d["beta"]), L.ptr(mean), L.ptr(var),
                                             relu6, BN_EPS, L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(ws), nb, L.stream_ptr()), "bn bwd")
    got = {"y": y, "mean": mean, "var": var, "dx": dx, "dgamma": dg, "dbeta": db}
    devs = {k: rel_dev(got[k].cpu().numpy(), ref[k]) for k in ref}
    print("batchnorm P=%d relu6=%d: bound %.3g, deviations %s" % (P, relu6, bound, {k: "%.3g" % v for k, v in devs.items()}))
    for k, v in devs.items():
        assert v <= bound, (k, v, bound)
    assert rel_dev(var.cpu().numpy()[5:6], ref["var"][5:6]) < 1e-3            # the channel the naive formula gets wrong
    # moving statistics after one step, against the formula (float64 batch statistics)
    want_m = mm0.astype(np.float64) * MOM32 + ref["mean"] * ONE_MINUS_MOM32
    want_v = mv0.astype(np.float64) * MOM32 + ref["var"] * P / (P - 1) * ONE_MINUS_MOM32
    assert np.allclose(d["mm"].cpu().numpy(), want_m, rtol=5e-7, atol=1e-9) and np.allclose(d["mv"].cpu().numpy(), want_v, rtol=5e-7, atol=0)


# ---- GPU: the whole span ---------------------------------------------------------------------------------------------------------
IMG, BATCH = 80, 3


def targets(hp, B, seed):
    anchors = bo.generate_anchors(hp)
    A = len(anchors)
    rng = np.random.RandomState(seed)
    gt = cases.gt_boxes(rng, B, G=8, n_valid=5)
    labels = np.full((B, 8), -1, np.int32)
    labels[:, :5] = rng.randint(1, 21, size=(B, 5))
    rp = rng.randint(1, 1280, size=(B, A)).astype(np.int32)
    rn = rng.randint(1, 2560, size=(B, A)).astype(np.int32)
    d, lab = train_utils.calculate_rpn_actual_outputs(anchors, gt, labels, hp, random_pos=rp, random_neg=rn)
    return np.asarray(d), np.asarray(lab)


def span_graph(x0, wts, first, deltas, labels, training, dtype):
    """The span from conv `first` up, the RPN head and both losses in torch; x0 (B,F,F,C): the input of `first`.
    -> (leaf parameters, reg loss, cls loss, smallest distance of a ReLU6 input to 0 or 6)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)
    params, margin = {}, np.inf
    x = t(x0).permute(0, 3, 1, 2)
    block_in = None
    for name in SPAN[SPAN.index(first):]:
        bn = wts[name + "_BN"]
        params[name] = {"kernel": t(wts[name]["kernel"]).requires_grad_(True)}
        params[name + "_BN"] = {"gamma": t(bn["gamma"]).requires_grad_(True), "beta": t(bn["beta"]).requires_grad_(True)}
        k = params[name]["kernel"]
        if name.endswith("depthwise"):
            z = TF.conv2d(x, k.permute(2, 3, 0, 1), padding=1, groups=k.shape[2])
        else:
            if name.endswith("expand"):
                block_in = x
            z = TF.conv2d(x, k.permute(3, 2, 0, 1))
        y = TF.batch_norm(z, None if training else t(bn["mean"]), None if training else t(bn["var"]), params[name + "_BN"]["gamma"],
                          params[name + "_BN"]["beta"], training=training, eps=BN_EPS)
        if name.endswith("project"):
            x = y + block_in if y.shape[1] == block_in.shape[1] else y
        else:
            pre = y.detach().to(torch.float64).numpy()
            margin = min(margin, np.abs(pre).min(), np.abs(pre - 6.0).min())
            x = TF.hardtanh(y, 0.0, 6.0)
    for name in HEAD_LAYERS:
        params[name] = {"kernel": t(wts[name]["kernel"]).requires_grad_(True), "bias": t(wts[name]["bias"]).requires_grad_(True)}
    s = torch.relu(TF.conv2d(x, params["rpn_conv"]["kernel"].permute(3, 2, 0, 1), params["rpn_conv"]["bias"], padding=1)).permute(0, 2, 3, 1)
    reg = s @ params["rpn_reg"]["kernel"][0, 0] + params["rpn_reg"]["bias"]
    cls = torch.sigmoid(s @ params["rpn_cls"]["kernel"][0, 0] + params["rpn_cls"]["bias"])
    yt = t(deltas)
    a = (reg.reshape(reg.shape[0], -1, 4) - yt).abs()
    q = torch.clamp(a, max=1.0)
    pos = (yt != 0).any(-1).to(dtype)
    r = (pos * (0.5 * q * q + (a - q)).sum(-1)).sum() / torch.clamp(pos.sum(), min=1.0)
    lt = t(labels)
    keep = lt != -1
    pc = torch.clamp(cls[keep], EPS32, CLIP_HI)
    c = -(lt[keep] * torch.log(pc + EPS32) + (1 - lt[keep]) * torch.log(1 - pc + EPS32)).mean()
    return params, r, c, margin


def span_weights(hp, seed):
    """Synthetic weights whose ReLU6 BatchNorms in the span sit at beta ~ 3, gamma ~ 1: both tails clamp (about 0.1 % each) and few
    inputs come near 0 or 6."""
    w = synthetic_weights("mobilenet_v2", hp, seed=1)
    rng = np.random.RandomState(seed)
    for name in SPAN:
        C = w[name + "_BN"]["gamma"].shape[0]
        if not name.endswith("project"):
            w[name + "_BN"]["beta"] = rng.uniform(2.7, 3.3, C).astype(np.float32)
        w[name]["kernel"] = (w[name]["kernel"] * rng.uniform(0.9, 1.1, w[name]["kernel"].shape)).astype(np.float32)
    return w


@pytest.fixture(scope="module")
def span_case(lib):
    """One model (layer-by-layer graph, so that block inputs can be read), one batch, and weights drawn so that no ReLU6 input of
    the float64 run from block_7_expand lies within 1e-4 of 0 or 6; the float64 / float32 torch runs of that graph."""
    hp = hp_for(IMG)
    model = RPNModel("mobilenet_v2", hp, precision="f32", max_batch=BATCH, keep_activations=True)
    rng = np.random.RandomState(71)
    imgs = rng.uniform(0, 1, size=(BATCH, IMG, IMG, 3)).astype(np.float32)
    deltas, labels = targets(hp, BATCH, 71)
    model.set_weights(span_weights(hp, 0))
    model.predict_on_batch(imgs)
    acts = {n: model.get_activation(n).cpu().numpy() for n in ("block_6_project", "block_11_project", "block_10_project")}
    for seed in range(40):
        w = span_weights(hp, seed)
        p64, r, c, margin = span_graph(acts["block_6_project"], w, "block_7_expand", deltas, labels, True, torch.float64)
        if margin > 1e-4:
            break
    else:
        pytest.fail("no seed keeps the ReLU6 inputs away from 0 and 6")
    (r + c).backward()
    p32, r32, c32, _ = span_graph(acts["block_6_project"], w, "block_7_expand", deltas, labels, True, torch.float32)
    (r32 + c32).backward()
    return dict(hp=hp, model=model, imgs=imgs, deltas=deltas, labels=labels, w=w, p64=p64, p32=p32, losses64=(r.item(), c.item()),
                losses32=(r32.item(), c32.item()), x6=acts["block_6_project"])


def grad_devs(grads, ref):
    """{(layer, key): deviation relative to max |reference|}.  A project BatchNorm's beta has NO gradient in exact arithmetic (a
    per-channel constant in front of a conv + BatchNorm is removed by that BatchNorm's mean): its float64 gradient is rounding noise,
    so its error is measured against the same layer's gamma gradient."""
    out = {}
    for name, d in ref.items():
        for key, leaf in d.items():
            g64 = leaf.grad.detach().to(torch.float64).numpy()
            scale = np.abs(g64).max()
            if name.endswith("project_BN") and key == "beta":
                scale = np.abs(d["gamma"].grad.detach().to(torch.float64).numpy()).max()
            got = grads[name][key] if isinstance(grads[name][key], np.ndarray) else grads[name][key].grad.detach().to(torch.float64).numpy()
            out[(name, key)] = float(np.abs(np.asarray(got, np.float64) - g64).max() / scale)
    return out


def fresh(case, first):
    m = case["model"]
    m.set_weights(case["w"])
    m.compile(train_backbone_from=first)
    return m


@pytest.mark.gpu
def test_whole_span_gradients_match_float64_autograd(lib, span_case):
    """Every kernel, gamma and beta gradient from block_7_expand up, and the three losses, against torch float64 autograd of the
    same graph; bound 4 x the largest deviation torch float32 autograd shows on it.  100 % of the elements are compared."""
    case = span_case
    m = fresh(case, "block_7_expand")
    losses = m.train_on_batch(case["imgs"], (case["deltas"], case["labels"]))
    grads = m.get_gradients()
    assert set(grads) == set(case["p64"])
    r, c = case["losses64"]
    r32, c32 = case["losses32"]
    lbound = 4.0 * max(abs(r32 - r) / r, abs(c32 - c) / c, float(np.finfo(np.float32).eps))
    for got, want in zip(losses, (r + c, r, c)):
        assert abs(got - want) <= lbound * abs(want), (losses, r, c, lbound)
    t32 = grad_devs({n: d for n, d in case["p32"].items()}, case["p64"])
    bound = 4.0 * max(t32.values())
    devs = grad_devs(grads, case["p64"])
    worst = max(devs, key=devs.get)
    print("whole span: torch float32 worst %.3g -> bound %.3g; this step's worst %.3g at %s" % (max(t32.values()), bound, devs[worst], worst))
    for key, v in devs.items():
        assert v <= bound, (key, v, bound)
    # the layers below block_7_expand are frozen
    k = np.empty((1, 1, 192, 64), np.float32)
    st = lib.rpn_head_trainer_get_gradient(m._t, b"block_6_project", k.ctypes.data_as(L.c_float_p), None, L.stream_ptr())
    assert st == L.RPN_ERR_INVALID and b"frozen" in lib.rpn_last_error()
    assert m.trained_layers() == SPAN + HEAD_LAYERS


@pytest.mark.gpu
def test_truncated_span_matches_float64_autograd(lib, span_case):
    """Training from block_12_expand on the span's own weights.  The layers below it now run frozen (BatchNorm folded, inference mode),
    so block_12 sees another input than in a run from block_7_expand (batch statistics there); here the truncated run is checked on
    ITS input: gradients against torch float64 autograd of the truncated graph fed with the handle's block_11_project, same bound
    rule, and that only the four convs above train.  The bits of the two runs are compared in the next test."""
    case = span_case
    m = fresh(case, "block_12_expand")
    m.predict_on_batch(case["imgs"])
    x11 = m.get_activation("block_11_project").cpu().numpy()
    losses = m.train_on_batch(case["imgs"], (case["deltas"], case["labels"]))
    grads = m.get_gradients()
    p64, r, c, _ = span_graph(x11, case["w"], "block_12_expand", case["deltas"], case["labels"], True, torch.float64)
    (r + c).backward()
    p32, r32, c32, _ = span_graph(x11, case["w"], "block_12_expand", case["deltas"], case["labels"], True, torch.float32)
    (r32 + c32).backward()
    assert set(grads) == set(p64) and len(grads) == 4 * 2 + 3
    t32 = grad_devs(p32, p64)
    bound = 4.0 * max(t32.values())
    devs = grad_devs(grads, p64)
    worst = max(devs, key=devs.get)
    print("span from block_12_expand: torch float32 worst %.3g -> bound %.3g; this step's worst %.3g at %s"
          % (max(t32.values()), bound, devs[worst], worst))
    for key, v in devs.items():
        assert v <= bound, (key, v, bound)
    assert abs(losses[0] - (r + c).item()) <= 1e-5 * abs((r + c).item())
    st = lib.rpn_head_trainer_get_bn_gradient(m._t, b"block_11_project_BN", None, None, None)
    assert st == L.RPN_ERR_INVALID


@pytest.mark.gpu
def test_truncated_run_shares_bits_with_the_full_run(lib, span_case):
    """The layers trained from block_12_expand get the same bits as in a run from block_7_expand: first step, same images, targets
    and weights.  Blocks 7-11 run with batch statistics in the one run and folded moving statistics in the other, so the two runs
    share block_12's input only where that input does not depend on the statistics: the weights here give block_10_project_BN
    gamma 0 (its output is its beta, in either mode) and block_11_project_BN gamma 0 and beta 0 (block 11 adds an exact zero).
    block_12_expand then sees a per-channel constant; from block_12_depthwise up ('same' padding) everything varies again."""
    case = span_case
    w = {n: dict(d) for n, d in case["w"].items()}
    b10 = np.random.RandomState(5).uniform(0.25, 1.0, 96).astype(np.float32)
    w["block_10_project_BN"].update(gamma=np.zeros(96, np.float32), beta=b10)
    w["block_11_project_BN"].update(gamma=np.zeros(96, np.float32), beta=np.zeros(96, np.float32))
    m = case["model"]
    runs = {}
    for first in ("block_7_expand", "block_12_expand"):
        m.set_weights(w)
        m.compile(train_backbone_from=first)
        if first == "block_12_expand":                              # the frozen prefix hands block 12 exactly beta
            m.predict_on_batch(case["imgs"])
            x11 = m.get_activation("block_11_project").cpu().numpy()
            assert np.array_equal(x11, np.broadcast_to(b10, x11.shape))
        losses = m.train_on_batch(case["imgs"], (case["deltas"], case["labels"]))
        grads = {(n, k): v.tobytes() for n, d in m.get_gradients().items() for k, v in d.items()}
        runs[first] = (losses, grads, state_bytes(m), m.get_gradients())
    full, cut = runs["block_7_expand"], runs["block_12_expand"]
    assert len(cut[1]) == 4 * 3 + 3 * 2 and len(cut[2]) == 4 * 5 + 3 * 2
    assert cut[0] == full[0]
    for key in cut[1]:
        assert cut[1][key] == full[1][key], key
    for key in cut[2]:
        assert cut[2][key] == full[2][key], key
    for name in SPAN[SPAN.index("block_12_depthwise"):]:            # and the compared gradients are no zeros
        assert np.abs(cut[3][name]["kernel"]).max() > 0 and np.abs(cut[3][name + "_BN"]["gamma"]).max() > 0, name
        assert cut[2][(name, "kernel")] != w[name]["kernel"].tobytes(), name


def state_bytes(m):
    return {(n, k): v.tobytes() for n, d in m.get_weights().items() for k, v in d.items()}


@pytest.mark.gpu
def test_span_step_is_deterministic(lib, span_case):
    case = span_case
    runs = []
    for _ in range(2):
        m = fresh(case, "block_7_expand")
        losses = [m.train_on_batch(case["imgs"], (case["deltas"], case["labels"])) for _ in range(3)]
        runs.append((losses, state_bytes(m)))
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1]
    w0 = case["w"]
    moved = [n for n in SPAN if runs[0][1][(n, "kernel")] != w0[n]["kernel"].tobytes()]
    assert moved == list(SPAN)                                      # every trained kernel took the step
    assert all(runs[0][1][(n + "_BN", "mean")] != w0[n + "_BN"]["mean"].tobytes() for n in SPAN)


@pytest.mark.gpu
def test_evaluation_uses_the_moving_statistics_and_changes_nothing(lib, span_case):
    case = span_case
    m = fresh(case, "block_7_expand")
    before = state_bytes(m)
    ev = m.test_on_batch(case["imgs"], (case["deltas"], case["labels"]))
    assert state_bytes(m) == before and m.train_steps() == 0
    _, r, c, _ = span_graph(case["x6"], case["w"], "block_7_expand", case["deltas"], case["labels"], False, torch.float64)
    for got, want in zip(ev, ((r + c).item(), r.item(), c.item())):
        assert abs(got - want) <= 1e-5 * abs(want), (ev, r.item(), c.item())
    tr = m.train_on_batch(case["imgs"], (case["deltas"], case["labels"]))
    r_t, c_t = case["losses64"]
    assert abs(tr[0] - ev[0]) > 1e-3 * abs(ev[0])                   # training-mode and inference-mode BatchNorm differ on this batch
    assert abs(tr[0] - (r_t + c_t)) < abs(tr[0] - ev[0])
    # one step moved the moving statistics by the formula
    bn = m.get_weights()["block_7_expand_BN"]
    w0 = case["w"]["block_7_expand_BN"]
    z = TF.conv2d(torch.tensor(case["x6"].astype(np.float64)).permute(0, 3, 1, 2),
                  torch.tensor(case["w"]["block_7_expand"]["kernel"].astype(np.float64)).permute(3, 2, 0, 1))
    n = z.shape[0] * z.shape[2] * z.shape[3]
    bm, bv = z.mean((0, 2, 3)).numpy(), z.var((0, 2, 3), unbiased=False).numpy()
    assert np.allclose(bn["mean"], w0["mean"].astype(np.float64) * MOM32 + bm * ONE_MINUS_MOM32, rtol=1e-6, atol=1e-8)
    assert np.allclose(bn["var"], w0["var"].astype(np.float64) * MOM32 + bv * n / (n - 1) * ONE_MINUS_MOM32, rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_inference_after_span_training(lib, span_case, tmp_path):
    case = span_case
    m = fresh(case, "block_7_expand")
    for _ in range(2):
        m.train_on_batch(case["imgs"], (case["deltas"], case["labels"]))
    reg, cls = m.predict_on_batch(case["imgs"])
    path = str(tmp_path / "trained.npz")
    RPNModel.save_weights(m.get_weights(), path)
    other = RPNModel("mobilenet_v2", case["hp"], precision="f32", max_batch=BATCH, keep_activations=True)
    other.set_weights(case["w"])
    done = other.load_weights(path)
    assert set(done) == set(SPAN + HEAD_LAYERS)
    reg2, cls2 = other.predict_on_batch(case["imgs"])
    assert reg.tobytes() == reg2.tobytes() and cls.tobytes() == cls2.tobytes()
    other.set_weights(case["w"])
    reg0, _ = other.predict_on_batch(case["imgs"])
    assert reg0.tobytes() != reg.tobytes()                          # (training changed what the handle computes)


@pytest.mark.gpu
def test_recompile_to_a_narrower_span_keeps_the_trained_layers(lib, span_case):
    """After steps from block_7_expand, compile(train_backbone_from="block_12_expand") with no inference in between: blocks 7-11 are
    frozen now and run on the handle, which must hold their TRAINED values -- the evaluation loss equals that of a fresh model given
    the trained weights, and differs from one whose blocks 7-11 went back to the original weights."""
    case = span_case
    batch = (case["imgs"], (case["deltas"], case["labels"]))
    m = fresh(case, "block_7_expand")
    m.compile(learning_rate=1e-3, train_backbone_from="block_7_expand")
    for _ in range(2):
        m.train_on_batch(*batch)
    trained = m.get_weights()
    m.compile(train_backbone_from="block_12_expand")
    ev = m.test_on_batch(*batch)
    assert {k: v.tobytes() for k, v in m.get_weights()["block_12_expand_BN"].items()} == \
        {k: v.tobytes() for k, v in trained["block_12_expand_BN"].items()}
    other = RPNModel("mobilenet_v2", case["hp"], precision="f32", max_batch=BATCH, keep_activations=True)   # the same graph as m's
    other.set_weights(case["w"])
    other.set_weights(trained, partial=True)
    other.compile(train_backbone_from="block_12_expand")
    assert other.test_on_batch(*batch) == ev
    stale = dict(trained, **{n: case["w"][n] for n in case["w"] if n.startswith(("block_7", "block_8", "block_9", "block_10", "block_11"))})
    other.set_weights(stale, partial=True)
    other.compile(train_backbone_from="block_12_expand")
    assert other.test_on_batch(*batch) != ev
    # and back to head-only: the whole trained span runs on the handle
    m.compile()
    ev_head = m.test_on_batch(*batch)
    other.set_weights(trained, partial=True)
    other.compile()
    assert other.test_on_batch(*batch) == ev_head


@pytest.mark.gpu
def test_fit_from_block11_reduces_the_loss(lib, span_case):
    case = span_case
    m = case["model"]
    m.set_weights(case["w"])
    m.compile(learning_rate=1e-3, train_backbone_from="block_11_expand")
    assert m.trained_layers()[0] == "block_11_expand" and len(m.trained_layers()) == 10

    def gen():
        while True:
            yield case["imgs"], (case["deltas"], case["labels"])
    hist = m.fit(gen(), steps_per_epoch=4, epochs=3)
    assert hist["loss"][-1] < hist["loss"][0]
