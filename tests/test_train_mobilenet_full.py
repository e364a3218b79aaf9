"""Training of the whole MobileNetV2 backbone, ``compile(train_backbone=True)``: the stem Conv1, expanded_conv, the stride-2 blocks and
the stride-16 span, each conv with its BatchNorm in training mode, and the head -- the reference's trainer.py trains its Keras model
with a trainable base model.  The three backward kernels this needs beside those of test_train_mobilenet.py (depthwise 3x3 stride-2
data and weight gradient, the stem's weight gradient) and the whole-model step.

Oracles: numpy / torch on the CPU, as in test_train_mobilenet.py, whose helpers and constants this file shares.  Integer-valued inputs
make the kernels exact in float32 whatever the summation order; the whole-model gradients are compared against torch float64 autograd
and bounded by 4 x the largest deviation torch float32 shows on the same graph (relative to max |reference| of each tensor).

Padding of the stride-2 layers: Keras ZeroPadding2D(correct_pad) + a 'valid' conv -- per spatial dim (0, 1) on an even side, (1, 1)
on an odd one.
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
import test_train_mobilenet as sib  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, RPNModel, synthetic_weights  # noqa: E402

TF = torch.nn.functional
CONVS = (("Conv1", "expanded_conv_depthwise", "expanded_conv_project")
         + tuple("block_%d_%s" % (b, p) for b in range(1, 13) for p in ("expand", "depthwise", "project")) + ("block_13_expand",))
STRIDE2 = ("Conv1", "block_1_depthwise", "block_3_depthwise", "block_6_depthwise")
NEW_SYMBOLS = ("rpn_model_trainer_create_full", "rpn_dwconv3x3_s2_dgrad", "rpn_dwconv3x3_s2_wgrad_workspace_bytes", "rpn_dwconv3x3_s2_wgrad",
               "rpn_conv3x3_s2_cin3_wgrad_workspace_bytes", "rpn_conv3x3_s2_cin3_wgrad")


def bn_of(name):
    """The BatchNorm layer behind conv `name` (Keras names: the stem's is bn_Conv1)."""
    return "bn_Conv1" if name == "Conv1" else name + "_BN"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


# ---- CPU: the Python surface and the ABI ----------------------------------------------------------------------------------
def test_train_backbone_trains_all_forty_convs(lib, tmp_path):
    assert len(CONVS) == 40
    hp = sib.hp_for(224)
    m = RPNModel("mobilenet_v2", hp, max_batch=1)
    w = synthetic_weights("mobilenet_v2", hp, seed=3)
    for name in HEAD_LAYERS:
        m._head[name] = (w[name]["kernel"], w[name]["bias"])
    for name in CONVS:
        m._mn[name] = dict({"kernel": w[name]["kernel"]}, **w[bn_of(name)])
    m.compile(train_backbone=True)
    assert m.trained_layers() == CONVS + HEAD_LAYERS
    got = m.get_weights()
    bns = {bn_of(c) for c in CONVS}
    assert len(bns) == 40 and set(got) == set(CONVS) | set(HEAD_LAYERS) | bns
    for name in HEAD_LAYERS:
        assert np.array_equal(got[name]["kernel"], w[name]["kernel"]) and np.array_equal(got[name]["bias"], w[name]["bias"]), name
    for name in CONVS:
        assert set(got[name]) == {"kernel"} and np.array_equal(got[name]["kernel"], w[name]["kernel"]), name
        assert set(got[bn_of(name)]) == {"gamma", "beta", "mean", "var"}
        for key in ("gamma", "beta", "mean", "var"):
            assert np.array_equal(got[bn_of(name)][key], w[bn_of(name)][key]), (name, key)
    path = str(tmp_path / "w.npz")
    RPNModel.save_weights(got, path)
    data = np.load(path)
    assert np.array_equal(data["Conv1/kernel"], w["Conv1"]["kernel"])
    assert np.array_equal(data["expanded_conv_depthwise_BN/var"], w["expanded_conv_depthwise_BN"]["var"])
    # the default changes nothing, and names below block_7_expand stay refused where they were
    m.compile(train_backbone=False)
    assert m.trained_layers() == HEAD_LAYERS
    with pytest.raises(ValueError, match="head only"):
        m.compile(train_backbone_from="Conv1")


def test_train_backbone_on_vgg16_is_block1_conv1(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    a, b = RPNModel("vgg16", hp, max_batch=1), RPNModel("vgg16", hp, max_batch=1)
    a.compile(train_backbone=True)
    b.compile(train_backbone_from="block1_conv1")
    assert a.trained_layers() == b.trained_layers() and len(a.trained_layers()) == 13 + 3


def test_train_backbone_and_train_backbone_from_exclude_each_other(lib):
    m = RPNModel("mobilenet_v2", sib.hp_for(80), max_batch=1)
    with pytest.raises(ValueError, match="train_backbone_from"):
        m.compile(train_backbone=True, train_backbone_from="block_7_expand")
    v = RPNModel("vgg16", bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14), max_batch=1)
    with pytest.raises(ValueError, match="train_backbone_from"):
        v.compile(train_backbone=True, train_backbone_from="block1_conv1")


def test_trainer_create_full_refuses_null_arguments(lib):
    m = RPNModel("mobilenet_v2", sib.hp_for(80), max_batch=1)
    t = L.vp(0)
    assert lib.rpn_model_trainer_create_full(None, ctypes.byref(t)) == L.RPN_ERR_INVALID
    assert lib.rpn_model_trainer_create_full(m._h, None) == L.RPN_ERR_INVALID
    assert lib.rpn_model_trainer_create_full(m._h, ctypes.byref(t)) == L.RPN_OK and t
    k = np.empty((3, 3, 3, 32), np.float32)
    assert lib.rpn_head_trainer_get_layer(t, b"Conv1", k.ctypes.data_as(L.c_float_p), None, None) == L.RPN_ERR_INVALID
    assert b"never set" in lib.rpn_last_error()                      # (trained, not frozen)
    lib.rpn_head_trainer_destroy(t)


def test_new_entries_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in L.exported_symbols(), name
        assert hasattr(raw, name), name
    assert lib.rpn_abi_version() == 1


def test_new_entries_validate_before_device_use(lib):
    p, q, ws = L.vp(64), L.vp(68), 1 << 22                           # never dereferenced: validation comes first
    assert lib.rpn_dwconv3x3_s2_wgrad_workspace_bytes(2, 10, 10, 96) > 0 and lib.rpn_dwconv3x3_s2_wgrad_workspace_bytes(2, 10, 10, 6) == 0
    assert lib.rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(2, 10, 10, 32) > 0 and lib.rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(2, 0, 10, 32) == 0
    # C = 6
    assert lib.rpn_dwconv3x3_s2_dgrad(p, p, 1, 5, 5, 6, p, None) == L.RPN_ERR_INVALID
    assert b"multiple of 4" in lib.rpn_last_error()
    assert lib.rpn_dwconv3x3_s2_wgrad(p, p, 1, 5, 5, 6, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_s2_cin3_wgrad(p, p, 1, 5, 5, 6, p, p, ws, None) == L.RPN_ERR_INVALID
    assert b"multiple of 4" in lib.rpn_last_error()
    # zero sizes and null pointers
    assert lib.rpn_dwconv3x3_s2_dgrad(p, p, 0, 5, 5, 8, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_dwconv3x3_s2_wgrad(p, p, 1, 5, 0, 8, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_s2_cin3_wgrad(p, p, 1, 0, 5, 32, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_dwconv3x3_s2_dgrad(p, None, 1, 5, 5, 8, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_dwconv3x3_s2_wgrad(None, p, 1, 5, 5, 8, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_s2_cin3_wgrad(p, p, 1, 5, 5, 32, None, p, ws, None) == L.RPN_ERR_INVALID
    # a pointer 4 bytes off 16-byte alignment
    assert lib.rpn_dwconv3x3_s2_dgrad(p, q, 1, 5, 5, 8, p, None) == L.RPN_ERR_INVALID
    assert b"16-byte aligned" in lib.rpn_last_error()
    assert lib.rpn_dwconv3x3_s2_wgrad(p, p, 1, 5, 5, 8, q, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_s2_cin3_wgrad(p, q, 1, 5, 5, 32, p, p, ws, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_s2_cin3_wgrad(p, p, 1, 5, 5, 32, p, q, ws, None) == L.RPN_ERR_INVALID
    assert b"16-byte aligned" in lib.rpn_last_error()
    # a workspace that is too small
    assert lib.rpn_dwconv3x3_s2_wgrad(p, p, 1, 5, 5, 8, p, None, 0, None) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_dwconv3x3_s2_wgrad(p, p, 1, 5, 5, 8, p, p, lib.rpn_dwconv3x3_s2_wgrad_workspace_bytes(1, 5, 5, 8) - 1, None) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_conv3x3_s2_cin3_wgrad(p, p, 1, 5, 5, 32, p, p, 16, None) == L.RPN_ERR_WORKSPACE


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_new_entries_need_a_device(lib):
    p, ws = L.vp(64), 1 << 22
    assert lib.rpn_dwconv3x3_s2_dgrad(p, p, 1, 5, 5, 8, p, None) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()
    assert lib.rpn_dwconv3x3_s2_wgrad(p, p, 1, 5, 5, 8, p, p, ws, None) == L.RPN_ERR_NO_DEVICE
    assert lib.rpn_conv3x3_s2_cin3_wgrad(p, p, 1, 5, 5, 32, p, p, ws, None) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()


def test_depthwise_and_tree_kernel_budgets(lib):
    """The stride-1 / stride-2 instances of the one depthwise backward pair, the two slab trees and the stem's weight gradient, each at
    what its separate predecessor (dwconv3x3[_s2]_dgrad_kernel, dwconv3x3[_s2]_wgrad_partial_kernel, leaf_tree_kernel, stem_tree_kernel)
    compiled to: registers, SGPR spills (the trees' go to register lanes, not to memory) and LDS; no scratch."""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    budgets = {"dwconv3x3_dgrad_kernel<1>": (38, 0, 0), "dwconv3x3_dgrad_kernel<2>": (36, 0, 0),
               "dwconv3x3_wgrad_partial_kernel<1,16,16>": (68, 0, 36864), "dwconv3x3_wgrad_partial_kernel<2,8,32>": (70, 0, 36864),
               "slab_tree_kernel<1>": (39, 40, 0), "slab_tree_kernel<8>": (56, 500, 0),
               "conv3x3_s2_cin3_wgrad_partial_kernel": (139, 0, 36864)}
    for name, (vgpr, sspill, lds) in budgets.items():
        assert name in tab, name
        v, ss, vs, scratch, lds_b, _wg = tab[name]
        assert v <= vgpr and ss <= sspill and vs == 0 and scratch == 0 and lds_b <= lds, (name, tab[name])


# ---- GPU: single kernels, bit-exact on small integers -----------------------------------------------------------------------
def pad_s2(x):
    """Keras ZeroPadding2D(correct_pad(x, 3)) on an NCHW tensor: (0, 1) on an even side, (1, 1) on an odd one."""
    return TF.pad(x, (x.shape[3] % 2, 1, x.shape[2] % 2, 1))


def out_side(n):
    return (n + n % 2 + 1 - 3) // 2 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C", [(2, 10, 10, 96), (2, 9, 9, 144), (1, 7, 12, 8), (1, 1, 1, 4), (1, 2, 2, 4), (3, 63, 63, 192)])
def test_depthwise_stride2_backward_integer_bit_exact(lib, B, H, W, C):
    """(2, 9, 9, 144), (1, 7, 12, 8), (1, *, *, 4): channel counts that are no multiple of the weight gradient's 32-channel tile;
    (3, 63, 63, 192): 3072 output pixels in 32 leaves of 96, three turns of the 32 row lanes each."""
    rng = np.random.RandomState(B * H + W + C)
    OH, OW = out_side(H), out_side(W)
    x, dy, w = sib.ints(rng, (B, H, W, C)), sib.ints(rng, (B, OH, OW, C)), sib.ints(rng, (3, 3, C))
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    wt = torch.tensor(w.astype(np.float64), requires_grad=True)
    y = TF.conv2d(pad_s2(xt.permute(0, 3, 1, 2)), wt.permute(2, 0, 1).unsqueeze(1), stride=2, groups=C).permute(0, 2, 3, 1)
    assert tuple(y.shape) == (B, OH, OW, C)
    y.backward(torch.tensor(dy.astype(np.float64)))
    x_d, dy_d, w_d = sib.cuda(x), sib.cuda(dy), sib.cuda(w)
    dx_out = torch.full((B, H, W, C), 7.0, device="cuda")
    dw_out = torch.full((3, 3, C), 7.0, device="cuda")
    L.check(lib.rpn_dwconv3x3_s2_dgrad(L.ptr(dy_d), L.ptr(w_d), B, H, W, C, L.ptr(dx_out), L.stream_ptr()), "dw s2 dgrad")
    assert np.array_equal(dx_out.cpu().numpy(), xt.grad.numpy().astype(np.float32))
    nb = lib.rpn_dwconv3x3_s2_wgrad_workspace_bytes(B, H, W, C)
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    L.check(lib.rpn_dwconv3x3_s2_wgrad(L.ptr(x_d), L.ptr(dy_d), B, H, W, C, L.ptr(dw_out), L.ptr(ws), nb, L.stream_ptr()), "dw s2 wgrad")
    assert np.array_equal(dw_out.cpu().numpy(), wt.grad.numpy().astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cout", [(2, 10, 10, 32), (1, 9, 13, 32), (3, 100, 100, 32), (4, 92, 92, 32), (1, 6, 5, 40)])
def test_stem_weight_gradient_integer_bit_exact(lib, B, H, W, Cout):
    """(3, 100, 100, 32): 7500 output pixels, 32 leaves; (4, 92, 92, 32): 8464 pixels, 64 leaves -- the second level of the leaf tree;
    (1, 6, 5, 40): a channel count that is no multiple of the 32-channel tile."""
    rng = np.random.RandomState(B * H + W + Cout)
    OH, OW = out_side(H), out_side(W)
    x, dy = sib.ints(rng, (B, H, W, 3)), sib.ints(rng, (B, OH, OW, Cout))
    xt = torch.tensor(x.astype(np.float64))
    wt = torch.zeros((3, 3, 3, Cout), dtype=torch.float64, requires_grad=True)
    y = TF.conv2d(pad_s2(xt.permute(0, 3, 1, 2)), wt.permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1)
    assert tuple(y.shape) == (B, OH, OW, Cout)
    y.backward(torch.tensor(dy.astype(np.float64)))
    x_d, dy_d = sib.cuda(x), sib.cuda(dy)
    dw_out = torch.full((3, 3, 3, Cout), 7.0, device="cuda")
    nb = lib.rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(B, H, W, Cout)
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    L.check(lib.rpn_conv3x3_s2_cin3_wgrad(L.ptr(x_d), L.ptr(dy_d), B, H, W, Cout, L.ptr(dw_out), L.ptr(ws), nb, L.stream_ptr()), "stem wgrad")
    assert np.array_equal(dw_out.cpu().numpy(), wt.grad.numpy().astype(np.float32))


# ---- GPU: the whole-model step ---------------------------------------------------------------------------------------------------
# Image 36, batch 2: the sides run 36 -> 18 -> 9 -> 5 -> 3, the four stride-2 layers see even, even, odd, odd input sides, as at
# 500 -> 250 -> 125 -> 63 -> 32.
IMG, BATCH = 36, 2
WEIGHT_SEED = 12                    # found on the CPU (full_case recomputes the condition it was chosen for)


def full_graph(imgs, wts, deltas, labels, training, dtype):
    """The whole model in torch: the 40 convs, each with BatchNorm (+ a strict ReLU6), the RPN head and both losses.
    -> (leaf parameters, reg loss, cls loss, {conv: its output z}, {conv: its ReLU6 inputs, flattened})."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)
    params, zs, pres = {}, {}, {}
    x = t(imgs).permute(0, 3, 1, 2)
    block_in = None
    for name in CONVS:
        bn = wts[bn_of(name)]
        params[name] = {"kernel": t(wts[name]["kernel"]).requires_grad_(True)}
        params[bn_of(name)] = {"gamma": t(bn["gamma"]).requires_grad_(True), "beta": t(bn["beta"]).requires_grad_(True)}
        k = params[name]["kernel"]
        if name == "Conv1":
            z = TF.conv2d(pad_s2(x), k.permute(3, 2, 0, 1), stride=2)
        elif name.endswith("depthwise"):
            if name in STRIDE2:
                z = TF.conv2d(pad_s2(x), k.permute(2, 3, 0, 1), stride=2, groups=k.shape[2])
            else:
                z = TF.conv2d(x, k.permute(2, 3, 0, 1), padding=1, groups=k.shape[2])
        else:
            if name.endswith("expand"):
                block_in = x
            z = TF.conv2d(x, k.permute(3, 2, 0, 1))
        zs[name] = z.detach().to(torch.float64).numpy()
        y = TF.batch_norm(z, None if training else t(bn["mean"]), None if training else t(bn["var"]), params[bn_of(name)]["gamma"],
                          params[bn_of(name)]["beta"], training=training, eps=sib.BN_EPS)
        if name.endswith("project"):
            res = block_in is not None and y.shape == block_in.shape
            x = y + block_in if res else y
            block_in = None
        else:
            pres[name] = y.detach().to(torch.float64).numpy().ravel()
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
    pc = torch.clamp(cls[keep], sib.EPS32, sib.CLIP_HI)
    c = -(lt[keep] * torch.log(pc + sib.EPS32) + (1 - lt[keep]) * torch.log(1 - pc + sib.EPS32)).mean()
    return params, r, c, zs, pres


def full_weights(hp, seed):
    """Synthetic weights whose ReLU6 BatchNorms sit at beta ~ 3, gamma ~ 1 (both tails clamp, few inputs come near 0 or 6); `seed`
    jitters every kernel."""
    w = synthetic_weights("mobilenet_v2", hp, seed=1)
    rng = np.random.RandomState(seed)
    for name in CONVS:
        C = w[bn_of(name)]["gamma"].shape[0]
        if not name.endswith("project"):
            w[bn_of(name)]["beta"] = rng.uniform(2.7, 3.3, C).astype(np.float32)
        w[name]["kernel"] = (w[name]["kernel"] * rng.uniform(0.9, 1.1, w[name]["kernel"].shape)).astype(np.float32)
    return w


def full_inputs(hp):
    rng = np.random.RandomState(71)
    imgs = rng.uniform(0, 1, size=(BATCH, IMG, IMG, 3)).astype(np.float32)
    deltas, labels = sib.targets(hp, BATCH, 71)
    return imgs, deltas, labels


def relu6_margin(pre64, pre32):
    """(smallest distance of a float64 ReLU6 input to 0 or 6, largest |float32 - float64| over all ReLU6 inputs)."""
    a, b = np.concatenate(list(pre64.values())), np.concatenate([pre32[n] for n in pre64])
    return float(min(np.abs(a).min(), np.abs(a - 6.0).min())), float(np.abs(b - a).max())


def grad_devs(grads, ref, flat_beta):
    """{(layer, key): deviation relative to max |reference|}, as test_train_mobilenet.grad_devs: a BatchNorm beta that has NO gradient
    in exact arithmetic is measured against the same layer's gamma gradient (its float64 gradient is rounding noise).  That is every
    project BatchNorm's beta, as there, and the betas of `flat_beta`: the depthwise BatchNorms none of whose ReLU6 inputs clamps on
    this batch -- the ReLU6 is then the identity, and a per-channel constant in front of the 1x1 project conv + BatchNorm is removed by
    that BatchNorm's mean (at a 3 x 3 feature map a depthwise layer has 18 pixels per channel, and some layer clamps nowhere)."""
    out = {}
    for name, d in ref.items():
        for key, leaf in d.items():
            g64 = leaf.grad.detach().to(torch.float64).numpy()
            scale = np.abs(g64).max()
            if key == "beta" and (name.endswith("project_BN") or name in flat_beta):
                scale = np.abs(d["gamma"].grad.detach().to(torch.float64).numpy()).max()
            got = grads[name][key] if isinstance(grads[name][key], np.ndarray) else grads[name][key].grad.detach().to(torch.float64).numpy()
            out[(name, key)] = float(np.abs(np.asarray(got, np.float64) - g64).max() / scale)
    return out


@pytest.fixture(scope="module")
def full_case(lib):
    """One model (layer-by-layer graph), one batch, the torch float64 / float32 runs of the whole graph.  A ReLU6 input on 0 or 6 to
    within rounding flips a mask, and one flipped pixel shows in a weight gradient at this size: WEIGHT_SEED was chosen so that every
    ReLU6 input of the float64 run lies farther from 0 and 6 than 8 x the largest float32 - float64 difference of those inputs, and
    the condition is recomputed here."""
    hp = sib.hp_for(IMG)
    imgs, deltas, labels = full_inputs(hp)
    w = full_weights(hp, WEIGHT_SEED)
    p64, r, c, zs, pre64 = full_graph(imgs, w, deltas, labels, True, torch.float64)
    (r + c).backward()
    p32, r32, c32, _, pre32 = full_graph(imgs, w, deltas, labels, True, torch.float32)
    (r32 + c32).backward()
    margin, diff = relu6_margin(pre64, pre32)
    allpre = np.concatenate(list(pre64.values()))
    assert allpre.size > 300000 and (allpre <= 0).sum() > 0 and (allpre >= 6).sum() > 0    # the mask is exercised on both sides
    # depthwise layers that clamp nowhere: their beta gradient is zero but for rounding (grad_devs), and only theirs
    flat_beta = {bn_of(n) for n, v in pre64.items() if n.endswith("depthwise") and not ((v <= 0).any() or (v >= 6).any())}
    for n in pre64:
        g = {k: p64[bn_of(n)][k].grad.abs().max().item() for k in ("gamma", "beta")}
        assert (g["beta"] < 1e-9 * g["gamma"]) == (bn_of(n) in flat_beta), (n, g)
    assert margin > 8.0 * diff, "WEIGHT_SEED %d: a ReLU6 input %.3g from 0 or 6, float32 moves them by %.3g" % (WEIGHT_SEED, margin, diff)
    model = RPNModel("mobilenet_v2", hp, precision="f32", max_batch=BATCH, keep_activations=True)
    assert model.feature_map_shape == 3
    return dict(hp=hp, model=model, imgs=imgs, deltas=deltas, labels=labels, w=w, p64=p64, p32=p32, zs=zs, flat_beta=flat_beta,
                losses64=(r.item(), c.item()), losses32=(r32.item(), c32.item()))


def fresh(case, **kw):
    m = case["model"]
    m.set_weights(case["w"])
    m.compile(train_backbone=True, **kw)
    return m


@pytest.mark.gpu
def test_whole_model_gradients_match_float64_autograd(lib, full_case):
    """Every kernel, gamma and beta gradient of the 40 convs and the head, and the three losses, against torch float64 autograd of the
    same graph; bound 4 x the largest deviation torch float32 autograd shows on it.  100 % of the elements are compared.
    Measured on the MI355X: torch float32 worst 1.03e-5 (block_9_depthwise_BN beta, a layer where two or three values clamp), bound
    4.12e-5, this step's worst 1.07e-5 at the same tensor; losses within 1.5e-7 of float64 (bound 2.6e-6)."""
    case = full_case
    m = fresh(case)
    assert m.trained_layers() == CONVS + HEAD_LAYERS
    losses = m.train_on_batch(case["imgs"], (case["deltas"], case["labels"]))
    grads = m.get_gradients()
    assert set(grads) == set(case["p64"]) and len(grads) == 83
    r, c = case["losses64"]
    r32, c32 = case["losses32"]
    lbound = 4.0 * max(abs(r32 - r) / r, abs(c32 - c) / c, float(np.finfo(np.float32).eps))
    print("whole model: losses %s, float64 %s, bound %.3g" % (losses, (r + c, r, c), lbound))
    t32 = grad_devs(case["p32"], case["p64"], case["flat_beta"])
    bound = 4.0 * max(t32.values())
    devs = grad_devs(grads, case["p64"], case["flat_beta"])
    worst = max(devs, key=devs.get)
    print("whole model: torch float32 worst %.3g at %s -> bound %.3g; this step's worst %.3g at %s"
          % (max(t32.values()), max(t32, key=t32.get), bound, devs[worst], worst))
    for got, want in zip(losses, (r + c, r, c)):
        assert abs(got - want) <= lbound * abs(want), (losses, r, c, lbound)
    for key, v in devs.items():
        assert v <= bound, (key, v, bound)


@pytest.mark.gpu
def test_whole_model_step_is_deterministic(lib, full_case):
    """Two fresh trainers: byte-identical weights, moving statistics and (through the second step's update) Adam state after two steps."""
    case = full_case
    runs = []
    for _ in range(2):
        m = fresh(case)
        losses = [m.train_on_batch(case["imgs"], (case["deltas"], case["labels"])) for _ in range(2)]
        grads = {(n, k): v.tobytes() for n, d in m.get_gradients().items() for k, v in d.items()}
        runs.append((losses, sib.state_bytes(m), grads))
    assert runs[0] == runs[1]
    w0 = case["w"]
    assert [n for n in CONVS if runs[0][1][(n, "kernel")] != w0[n]["kernel"].tobytes()] == list(CONVS)      # every kernel took the step
    assert all(runs[0][1][(bn_of(n), "mean")] != w0[bn_of(n)]["mean"].tobytes() for n in CONVS)


@pytest.mark.gpu
def test_whole_model_evaluation_uses_the_moving_statistics_and_changes_nothing(lib, full_case):
    case = full_case
    batch = (case["imgs"], (case["deltas"], case["labels"]))
    m = fresh(case)
    before = sib.state_bytes(m)
    ev = m.test_on_batch(*batch)
    assert sib.state_bytes(m) == before and m.train_steps() == 0
    # inference-mode BatchNorm: the losses of the torch graph run with the moving statistics, within 4 x torch float32's own deviation
    _, r, c, _, _ = full_graph(case["imgs"], case["w"], case["deltas"], case["labels"], False, torch.float64)
    _, r32, c32, _, _ = full_graph(case["imgs"], case["w"], case["deltas"], case["labels"], False, torch.float32)
    r, c, r32, c32 = r.item(), c.item(), r32.item(), c32.item()
    lbound = 4.0 * max(abs(r32 - r) / r, abs(c32 - c) / c, float(np.finfo(np.float32).eps))
    print("whole model, evaluation: %s, float64 %s, bound %.3g" % (ev, (r + c, r, c), lbound))
    for got, want in zip(ev, (r + c, r, c)):
        assert abs(got - want) <= lbound * abs(want), (ev, r, c, lbound)
    tr = m.train_on_batch(*batch)
    r_t, c_t = case["losses64"]
    assert abs(tr[0] - ev[0]) > 1e-3 * abs(ev[0])                   # training-mode and inference-mode BatchNorm differ on this batch
    assert abs(tr[0] - (r_t + c_t)) < abs(tr[0] - ev[0])
    assert m.test_on_batch(*batch) != ev and m.train_steps() == 1   # (the step moved the model; an evaluation advances nothing)
    # one step moved the moving statistics by the formula: the stem and the three stride-2 depthwise convs
    got = m.get_weights()
    for name in STRIDE2:
        z = case["zs"][name]
        n = z.shape[0] * z.shape[2] * z.shape[3]
        bm, bv = z.mean((0, 2, 3)), z.var((0, 2, 3))
        bn, w0 = got[bn_of(name)], case["w"][bn_of(name)]
        assert np.allclose(bn["mean"], w0["mean"].astype(np.float64) * sib.MOM32 + bm * sib.ONE_MINUS_MOM32, rtol=1e-6, atol=1e-8), name
        assert np.allclose(bn["var"], w0["var"].astype(np.float64) * sib.MOM32 + bv * n / (n - 1) * sib.ONE_MINUS_MOM32, rtol=1e-6, atol=0), name


@pytest.mark.gpu
def test_inference_after_whole_model_training(lib, full_case, tmp_path):
    """After a step the handle runs the trained model: its float32 forward (BatchNorm refolded from the trained kernels, gamma, beta
    and the moved statistics) against the trainer's own evaluation outputs, within the float32 handle's 1e-5; and, as in
    test_inference_after_span_training, a fresh handle given the saved weights reproduces the predictions bit for bit."""
    case = full_case
    batch = (case["imgs"], (case["deltas"], case["labels"]))
    m = fresh(case)
    m.train_on_batch(*batch)
    _, (reg_t, cls_t) = m.test_on_batch(*batch, return_outputs=True)
    reg, cls = m.predict_on_batch(case["imgs"])
    d_reg, d_cls = np.abs(reg - reg_t.cpu().numpy()).max(), np.abs(cls - cls_t.cpu().numpy()).max()
    print("whole model, inference after a step: |reg - trainer's| %.3g, |cls - trainer's| %.3g" % (d_reg, d_cls))
    assert d_reg <= 1e-5 and d_cls <= 1e-5
    path = str(tmp_path / "trained.npz")
    RPNModel.save_weights(m.get_weights(), path)
    other = RPNModel("mobilenet_v2", case["hp"], precision="f32", max_batch=BATCH, keep_activations=True)
    other.set_weights(case["w"])
    done = other.load_weights(path)
    assert set(done) == set(CONVS + HEAD_LAYERS)
    reg2, cls2 = other.predict_on_batch(case["imgs"])
    assert reg.tobytes() == reg2.tobytes() and cls.tobytes() == cls2.tobytes()
    other.set_weights(case["w"])
    reg0, _ = other.predict_on_batch(case["imgs"])
    assert reg0.tobytes() != reg.tobytes()                          # (training changed what the handle computes)
    # the fused graph (one launch per inverted-residual block) takes the same layers
    fused = RPNModel("mobilenet_v2", case["hp"], precision="f32", max_batch=BATCH)
    fused.set_weights(case["w"])
    fused.compile(train_backbone=True)
    fused.train_on_batch(*batch)
    _, (reg_f, cls_f) = fused.test_on_batch(*batch, return_outputs=True)
    assert reg_f.cpu().numpy().tobytes() == reg_t.cpu().numpy().tobytes()        # the trainer does not depend on the handle's graph
    reg3, cls3 = fused.predict_on_batch(case["imgs"])
    assert np.abs(reg3 - reg_f.cpu().numpy()).max() <= 1e-5 and np.abs(cls3 - cls_f.cpu().numpy()).max() <= 1e-5


@pytest.mark.gpu
def test_whole_model_fit_reduces_the_loss(lib, full_case):
    case = full_case
    m = fresh(case, learning_rate=1e-3)
    assert len(m.trained_layers()) == 43

    def gen():
        while True:
            yield case["imgs"], (case["deltas"], case["labels"])
    hist = m.fit(gen(), steps_per_epoch=4, epochs=3)
    assert hist["loss"][-1] < hist["loss"][0]
