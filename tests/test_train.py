"""Training of the RPN head on a frozen backbone (trainer.py:54-69): losses, gradients, the 3x3 weight gradient, Adam, and the
trained head in inference.

Restatements used as oracles (float64), from TF 2.0.0's sources as recalled -- nothing here can run TF:
  cls_loss  utils/train_utils.py:146-162 + keras backend.binary_crossentropy(from_logits=False): p' = clip(p, eps, 1 - eps),
            -(t log(p' + eps) + (1 - t) log(1 - p' + eps)), eps = 1e-7 (float32), mean over the kept labels of the batch.
  reg_loss  utils/train_utils.py:164-185 + losses.huber_loss(delta=1) per element (no mean over the last axis in TF 2.0).
  Adam      training_ops ApplyAdam: alpha = lr sqrt(1 - b2^t) / (1 - b1^t), m += (g - m)(1 - b1), v += (g^2 - v)(1 - b2),
            w -= alpha m / (sqrt(v) + eps).
torch float64 autograd on the CPU is the gradient oracle.
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
from tf_rpn_amd.models import rpn_mobilenet_v2, rpn_vgg16  # noqa: E402
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, RPNModel, synthetic_weights  # noqa: E402
from tf_rpn_amd.utils import train_utils  # noqa: E402

EPS32 = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


# ---- float64 restatements ----------------------------------------------------------------------------------------------
def cls_loss64(y_true, y_pred):
    """utils/train_utils.py:146-162 with keras BinaryCrossentropy on probabilities (torch float64, differentiable)."""
    keep = y_true != -1
    t, p = y_true[keep], y_pred[keep]
    pc = torch.clamp(p, EPS32, CLIP_HI)
    bce = -(t * torch.log(pc + EPS32) + (1 - t) * torch.log(1 - pc + EPS32))
    return bce.mean()


def reg_loss64(y_true, y_pred):
    """utils/train_utils.py:164-185 with TF 2.0's per-element huber_loss (delta 1)."""
    y_pred = y_pred.reshape(y_pred.shape[0], -1, 4)
    a = (y_pred - y_true).abs()
    q = torch.clamp(a, max=1.0)
    loss = (0.5 * q * q + (a - q)).sum(-1)
    pos = (y_true != 0).any(-1).to(torch.float64)
    return (pos * loss).sum() / torch.clamp(pos.sum(), min=1.0)


def adam64(w, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-7):
    """ApplyAdam (training_ops), float64."""
    alpha = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    m = m + (g - m) * (1 - b1)
    v = v + (g * g - v) * (1 - b2)
    return w - alpha * m / (np.sqrt(v) + eps), m, v


def head64(X, wts, K):
    """rpn_conv (3x3 'same', ReLU) + rpn_reg (linear) | rpn_cls (sigmoid) on NHWC features, float64, leaf tensors returned."""
    params = {}
    for name in HEAD_LAYERS:
        params[name] = [torch.tensor(np.asarray(wts[name]["kernel"], np.float64), requires_grad=True),
                        torch.tensor(np.asarray(wts[name]["bias"], np.float64), requires_grad=True)]
    x = torch.tensor(np.asarray(X, np.float64)).permute(0, 3, 1, 2)
    k, b = params["rpn_conv"]
    s = torch.relu(torch.nn.functional.conv2d(x, k.permute(3, 2, 0, 1), b, padding=1)).permute(0, 2, 3, 1)
    reg = s @ params["rpn_reg"][0][0, 0] + params["rpn_reg"][1]
    cls = torch.sigmoid(s @ params["rpn_cls"][0][0, 0] + params["rpn_cls"][1])
    return params, reg, cls


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


# ---- CPU: the ABI and the Python surface --------------------------------------------------------------------------------
NEW_SYMBOLS = ("rpn_rpn_losses_workspace_bytes", "rpn_rpn_losses", "rpn_conv3x3_wgrad_workspace_bytes", "rpn_conv3x3_wgrad",
               "rpn_head_trainer_create", "rpn_head_trainer_destroy", "rpn_head_trainer_set_layer", "rpn_head_trainer_get_layer",
               "rpn_head_trainer_get_gradient", "rpn_head_trainer_step", "rpn_head_trainer_steps", "rpn_head_trainer_outputs")


def test_training_entries_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in L.exported_symbols(), name
        assert hasattr(raw, name), name


def test_training_entries_validate_before_device_use(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, L.vp)
    ws = (ctypes.c_ubyte * 8192)()
    wsp = ctypes.cast(ws, L.vp)
    assert lib.rpn_rpn_losses(None, p, p, p, 1, 4, p, None, None, wsp, 8192, None) == L.RPN_ERR_INVALID
    assert lib.rpn_rpn_losses(p, p, p, p, 0, 4, p, None, None, wsp, 8192, None) == L.RPN_ERR_INVALID
    assert lib.rpn_rpn_losses(p, p, p, p, 1, 4, p, None, None, None, 0, None) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_conv3x3_wgrad(p, None, 1, 4, 4, 8, 8, p, None, wsp, 8192, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_wgrad(p, p, 1, 4, 4, 6, 8, p, None, wsp, 8192, None) == L.RPN_ERR_INVALID     # Cin % 4
    assert lib.rpn_conv3x3_wgrad(p, p, 1, 4, 4, 8, 8, p, None, wsp, 16, None) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_head_trainer_create(None, None) == L.RPN_ERR_INVALID
    assert lib.rpn_head_trainer_step(None, p, 1, p, p, 1, 1e-5, 0.9, 0.999, 1e-7, p, None) == L.RPN_ERR_INVALID
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m = RPNModel("vgg16", hp, max_batch=2)
    m.compile()
    t = m._t
    assert lib.rpn_head_trainer_set_layer(t, b"block5_conv3", buf, buf) == L.RPN_ERR_INVALID
    assert b"frozen" in lib.rpn_last_error()
    assert lib.rpn_head_trainer_step(t, p, 3, p, p, 1, 1e-5, 0.9, 0.999, 1e-7, p, None) == L.RPN_ERR_INVALID   # batch > max_batch
    assert lib.rpn_head_trainer_step(t, p, 1, p, p, 1, 1e-5, 1.5, 0.999, 1e-7, p, None) == L.RPN_ERR_INVALID   # beta_1 >= 1
    assert lib.rpn_head_trainer_step(t, p, 1, p, p, 1, 1e-5, 0.9, 0.999, 1e-7, p, None) == L.RPN_ERR_INVALID   # head never set
    assert b"never set" in lib.rpn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_training_entries_need_a_device(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, L.vp)
    ws = (ctypes.c_ubyte * 8192)()
    wsp = ctypes.cast(ws, L.vp)
    assert lib.rpn_rpn_losses(p, p, p, p, 1, 4, p, None, None, wsp, lib.rpn_rpn_losses_workspace_bytes(1, 4), None) == L.RPN_ERR_NO_DEVICE
    need = lib.rpn_conv3x3_wgrad_workspace_bytes(1, 2, 2, 4, 4)
    big = (ctypes.c_ubyte * need)()
    assert lib.rpn_conv3x3_wgrad(p, p, 1, 2, 2, 4, 4, p, p, ctypes.cast(big, L.vp), need, None) == L.RPN_ERR_NO_DEVICE
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m = RPNModel("vgg16", hp, max_batch=1)
    m.compile()
    w = synthetic_weights("vgg16", hp, seed=3)
    for name in HEAD_LAYERS:            # (the inference handle's set_layer needs a device; the trainer's does not)
        m._head[name] = (w[name]["kernel"], w[name]["bias"])
        m._trainer_set(name)
    assert lib.rpn_head_trainer_step(m._t, p, 1, p, p, 1, 1e-5, 0.9, 0.999, 1e-7, p, None) == L.RPN_ERR_NO_DEVICE
    # the seeded head comes back unchanged without a device
    got = m.get_weights()
    for name in HEAD_LAYERS:
        assert np.array_equal(got[name]["kernel"], w[name]["kernel"]) and np.array_equal(got[name]["bias"], w[name]["bias"])
    with pytest.raises(RuntimeError):
        train_utils.cls_loss(np.zeros((1, 2, 2, 9), np.float32), np.zeros((1, 2, 2, 9), np.float32))


def test_compile_rejects_backbone_layers(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m = RPNModel("vgg16", hp, max_batch=1)
    for bad in (("rpn_conv", "rpn_cls", "rpn_reg", "block5_conv3"), ("rpn_cls", "rpn_reg"), "rpn_conv", ()):
        with pytest.raises(ValueError, match="frozen backbone"):
            m.compile(trainable=bad)
    m.compile(trainable=("rpn_reg", "rpn_conv", "rpn_cls"))
    with pytest.raises(RuntimeError, match="compile"):
        RPNModel("vgg16", hp, max_batch=1).train_on_batch(None, (None, None))


def test_loss_argument_forms():
    a, b = np.zeros(3), np.ones(3)
    assert train_utils._loss_args((a, b))[1] is b
    assert train_utils._loss_args(((a, b),))[0] is a
    with pytest.raises(TypeError):
        train_utils._loss_args((a,))


def test_wgrad_kernel_register_budget(lib):
    """No scratch; registers and LDS of the 3x3 weight-gradient kernel pinned (four waves of 112 registers, 40 KB of LDS:
    three workgroups per CU by LDS).  <false> is the head's instance; the backbone's <true> (the row of ones behind db) is held to the
    same budget by test_train_backbone.test_backbone_kernel_budgets."""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    budgets = {"conv3x3_wgrad_f32_kernel<false>": (128, 0, 40960), "rpn_loss_kernel": (64, 0, 8192),
               "head_wgrad_kernel<45>": (128, 0, 11520), "head_dgrad_kernel<45>": (160, 0, 2880), "adam_kernel": (48, 0, 0)}
    for name, (vgpr, sspill, lds) in budgets.items():
        assert name in tab, name
        v, ss, vs, scratch, l, _wg = tab[name]
        assert v <= vgpr and ss <= sspill and vs == 0 and scratch == 0 and l <= lds, (name, tab[name])
    # every instantiation rpn_head_trainer_create accepts (NC = 5K, K = 1 .. 12): in the library, no scratch, no spilled VGPR,
    # LDS = the dZ rows of one chunk (kChunkRows = 64 for the weight gradient, 16 for the data gradient).  head_dgrad_kernel runs
    # 512-thread workgroups: above 256 registers it cannot be launched, and <50> takes exactly 256
    for nc in range(5, 65, 5):
        for name, vgpr, lds in (("head_wgrad_kernel<%d>" % nc, 512, 64 * nc * 4), ("head_dgrad_kernel<%d>" % nc, 256, 16 * nc * 4)):
            assert name in tab, name
            v, _ss, vs, scratch, l, wg = tab[name]
            assert vs == 0 and scratch == 0 and v <= vgpr and l <= lds, (name, tab[name])
            assert wg == (256 if "wgrad" in name else 512), (name, wg)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def run_losses(reg_true, reg_pred, cls_true, cls_pred):
    B, A = reg_true.shape[:2]
    lib = L.lib()
    t = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() for v in (reg_true, reg_pred, cls_true, cls_pred)]
    out = torch.empty(2, device="cuda")
    gr = torch.empty((B, A, 4), device="cuda")
    gc = torch.empty((B, A), device="cuda")
    n = lib.rpn_rpn_losses_workspace_bytes(B, A)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    L.check(lib.rpn_rpn_losses(*[L.ptr(v) for v in t], B, A, L.ptr(out), L.ptr(gr), L.ptr(gc), L.ptr(ws), n, L.stream_ptr()),
            "rpn_rpn_losses")
    return out.cpu().numpy(), gr.cpu().numpy(), gc.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 8])
def test_losses_and_output_gradients(lib, B):
    hp = bo.get_hyper_params("vgg16")
    F, K = hp["feature_map_shape"], hp["anchor_count"]
    deltas, labels = targets(hp, B, seed=10 + B)
    rng = np.random.RandomState(B)
    reg_pred = (rng.standard_normal((B, F, F, 4 * K)) * 1.5).astype(np.float32)
    cls_pred = rng.uniform(0, 1, size=(B, F, F, K)).astype(np.float32)
    lab = labels.reshape(B, -1).copy()
    kept = np.flatnonzero(lab[0] != -1)
    cls_pred.reshape(B, -1)[0, kept[:4]] = [0.0, 1e-8, 1 - 1e-8, 1.0]        # the clip on both sides
    free = np.flatnonzero(lab[0] == -1)[0]
    lab[0, free] = 1.0                                                       # a positive whose deltas are exactly zero
    deltas[0, free] = 0.0
    labels = lab.reshape(labels.shape)
    assert (labels == 1).any() and (labels == 0).any()
    got, gr, gc = run_losses(deltas, reg_pred.reshape(B, -1, 4), labels.reshape(B, -1), cls_pred.reshape(B, -1))
    rt, rp = torch.tensor(deltas, dtype=torch.float64), torch.tensor(reg_pred, dtype=torch.float64, requires_grad=True)
    ct, cp = torch.tensor(labels, dtype=torch.float64), torch.tensor(cls_pred, dtype=torch.float64, requires_grad=True)
    r64, c64 = reg_loss64(rt, rp), cls_loss64(ct, cp)
    (r64 + c64).backward()
    assert abs(got[0] - r64.item()) <= 1e-6 * abs(r64.item()), (got, r64.item())
    assert abs(got[1] - c64.item()) <= 1e-6 * abs(c64.item()), (got, c64.item())
    g_reg, g_cls = rp.grad.numpy().reshape(B, -1, 4), cp.grad.numpy().reshape(B, -1)
    assert np.abs(gr - g_reg).max() <= 1e-6 * np.abs(g_reg).max()
    assert np.abs(gc - g_cls).max() <= 1e-6 * np.abs(g_cls).max()
    assert gc[0, kept[0]] == 0 and gc[0, kept[3]] == 0                    # clipped: no gradient
    # the public wrappers, both argument forms
    assert np.isclose(train_utils.reg_loss(deltas, reg_pred), got[0], rtol=0, atol=0)
    assert np.isclose(train_utils.reg_loss((deltas, reg_pred)), got[0], rtol=0, atol=0)
    assert train_utils.cls_loss(labels, cls_pred) == train_utils.cls_loss((labels, cls_pred)) == got[1]


@pytest.mark.gpu
def test_losses_without_valid_labels(lib):
    B, A = 2, 900
    rng = np.random.RandomState(0)
    deltas = np.zeros((B, A, 4), np.float32)
    got, gr, gc = run_losses(deltas, rng.standard_normal((B, A, 4)).astype(np.float32), np.full((B, A), -1, np.float32),
                             rng.uniform(size=(B, A)).astype(np.float32))
    assert got[0] == 0.0 and np.isnan(got[1])
    assert not gr.any() and not gc.any()


def wgrad(x, dy, with_db=True):
    lib = L.lib()
    B, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    xd, dyd = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    dw = torch.empty((3, 3, Cin, Cout), device="cuda")
    db = torch.empty((Cout,), device="cuda")
    n = lib.rpn_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Cout)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    L.check(lib.rpn_conv3x3_wgrad(L.ptr(xd), L.ptr(dyd), B, H, W, Cin, Cout, L.ptr(dw), L.ptr(db) if with_db else None, L.ptr(ws),
                                  n, L.stream_ptr()), "rpn_conv3x3_wgrad")
    return dw.cpu().numpy(), db.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,Cin", [(8, 31, 512), (1, 31, 512), (3, 32, 576)])
def test_wgrad_integer_bit_exact(lib, B, H, Cin):
    """Integers in [-4, 4]: every partial sum is an integer below 2^24, so float32 is exact and any race / hazard in the LDS
    pipeline or the split-K tree shows as a wrong bit.  The reference sums in float64 (exact for these magnitudes, < 2^53) and is
    compared as int64."""
    rng = np.random.RandomState(B * 7 + Cin)
    x = rng.randint(-4, 5, size=(B, H, H, Cin)).astype(np.float32)
    dy = rng.randint(-4, 5, size=(B, H, H, 512)).astype(np.float32)
    dw, db = wgrad(x, dy)
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    d2 = dy.astype(np.float64).reshape(-1, 512)
    ref = np.empty((3, 3, Cin, 512), np.int64)
    for r in range(3):
        for s in range(3):
            ref[r, s] = (xp[:, r:r + H, s:s + H, :].reshape(-1, Cin).T @ d2).astype(np.int64)
    assert np.array_equal(dw.astype(np.int64), ref)
    assert np.array_equal(db.astype(np.int64), dy.reshape(-1, 512).sum(0).astype(np.int64))


def make_model(backbone, hp, B, precision="f32", seed=1):
    mod = rpn_vgg16 if backbone == "vgg16" else rpn_mobilenet_v2
    model, _ = mod.get_model(hp, precision=precision, max_batch=B, seed=seed)
    return model


def batch(hp, B, seed):
    rng = np.random.RandomState(seed)
    imgs = rng.uniform(0, 1, size=(B, hp["img_size"], hp["img_size"], 3)).astype(np.float32)
    deltas, labels = targets(hp, B, seed)
    return imgs, deltas, labels


@pytest.mark.gpu
@pytest.mark.parametrize("backbone,B", [("vgg16", 1), ("vgg16", 8), ("mobilenet_v2", 2)])
def test_head_weight_gradients(lib, backbone, B):
    hp = bo.get_hyper_params(backbone)
    K = hp["anchor_count"]
    model = make_model(backbone, hp, B)
    w0 = model.get_weights()
    imgs, deltas, labels = batch(hp, B, seed=20 + B)
    model.compile()
    model.train_on_batch(imgs, (deltas, labels))
    grads = model.get_gradients()
    X = model.get_activation(model.tap_layer, batch=B).cpu().numpy()
    params, reg, cls = head64(X, w0, K)
    loss = reg_loss64(torch.tensor(deltas, dtype=torch.float64), reg) + cls_loss64(torch.tensor(labels, dtype=torch.float64), cls)
    loss.backward()
    for name in HEAD_LAYERS:
        for i, key in enumerate(("kernel", "bias")):
            g64 = params[name][i].grad.numpy()
            err = np.abs(grads[name][key] - g64).max()
            assert err <= 2e-5 * np.abs(g64).max(), (name, key, err, np.abs(g64).max())


@pytest.mark.gpu
def test_adam_steps_and_test_on_batch(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    model = make_model("vgg16", hp, 2)
    imgs, deltas, labels = batch(hp, 2, seed=31)
    lr = 1e-3
    model.compile(learning_rate=lr)
    w64 = {n: {k: v.astype(np.float64) for k, v in d.items()} for n, d in model.get_weights().items()}
    mv = {n: {k: (np.zeros_like(v), np.zeros_like(v)) for k, v in d.items()} for n, d in w64.items()}
    for t in (1, 2, 3):
        model.train_on_batch(imgs, (deltas, labels))
        g = model.get_gradients()
        for n in HEAD_LAYERS:
            for k in ("kernel", "bias"):
                w64[n][k], m, v = adam64(w64[n][k], g[n][k].astype(np.float64), *mv[n][k], t, lr)
                mv[n][k] = (m, v)
        if t in (1, 3):
            got = model.get_weights()
            for n in HEAD_LAYERS:
                for k in ("kernel", "bias"):
                    ref = w64[n][k]
                    assert np.abs(got[n][k] - ref).max() <= 1e-6 * np.abs(ref).max(), (t, n, k)
        before = model.get_weights()
        model.test_on_batch(imgs, (deltas, labels))
        assert model.train_steps() == t
        after = model.get_weights()
        assert all(np.array_equal(before[n]["kernel"], after[n]["kernel"]) for n in HEAD_LAYERS)


@pytest.mark.gpu
def test_train_step_is_deterministic(lib):
    hp = bo.get_hyper_params("vgg16")
    model = make_model("vgg16", hp, 8)
    w0 = model.get_weights()
    imgs, deltas, labels = batch(hp, 8, seed=41)
    runs = []
    for _ in range(2):
        model.compile()
        model.set_weights(w0, partial=True)
        losses = model.train_on_batch(imgs, (deltas, labels))
        runs.append((losses, model.get_weights()))
    assert runs[0][0] == runs[1][0]
    for n in HEAD_LAYERS:
        for k in ("kernel", "bias"):
            assert np.array_equal(runs[0][1][n][k], runs[1][1][n][k]), (n, k)


@pytest.mark.gpu
def test_five_steps_track_a_float64_replay_and_inference_sees_the_head(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    K, B, lr = hp["anchor_count"], 2, 1e-3
    model = make_model("vgg16", hp, B)
    imgs, deltas, labels = batch(hp, B, seed=51)
    w = model.get_weights()
    model.compile(learning_rate=lr)
    losses = [model.train_on_batch(imgs, (deltas, labels)) for _ in range(5)]
    X = model.get_activation(model.tap_layer, batch=B).cpu().numpy()
    # replay: the same five steps in float64 (the frozen features are the same every step)
    w64 = {n: {k: v.astype(np.float64) for k, v in d.items()} for n, d in w.items()}
    mv = {n: {k: (0.0, 0.0) for k in d} for n, d in w64.items()}
    losses64 = []
    dt, lt = torch.tensor(deltas, dtype=torch.float64), torch.tensor(labels, dtype=torch.float64)
    for t in range(1, 6):
        params, reg, cls = head64(X, w64, K)
        r, c = reg_loss64(dt, reg), cls_loss64(lt, cls)
        (r + c).backward()
        losses64.append([(r + c).item(), r.item(), c.item()])
        for n in HEAD_LAYERS:
            for i, k in enumerate(("kernel", "bias")):
                w64[n][k], m, v = adam64(w64[n][k], params[n][i].grad.numpy(), *mv[n][k], t, lr)
                mv[n][k] = (m, v)
    assert np.allclose(losses, losses64, rtol=1e-4, atol=0)
    # weights: Adam's update is lr g / (|g| + eps / sqrt(1 - b2^t)) for small |g| -- a slope of ~300 at lr 1e-3 -- so the float32
    # gradient's rounding (~1e-8 absolute on the rpn_conv kernel) reaches the weights amplified; measured 1.2e-4 of max|w| after five
    # steps, bounded at 2e-4
    got = model.get_weights()
    for n in HEAD_LAYERS:
        for k in ("kernel", "bias"):
            assert np.abs(got[n][k] - w64[n][k]).max() <= 2e-4 * np.abs(w64[n][k]).max(), (n, k)
    after, (reg, cls) = model.test_on_batch(imgs, (deltas, labels), return_outputs=True)
    params, reg64, cls64 = head64(X, w64, K)
    ref_total = (reg_loss64(dt, reg64) + cls_loss64(lt, cls64)).item()
    assert np.isclose(after[0], ref_total, rtol=1e-4)
    assert after[0] < losses64[0][0]
    # inference sees the trained head: f32 within 1e-5, f16x3 within the 1e-4 contract
    pred_reg, pred_cls = model.predict_on_batch(torch.from_numpy(imgs).cuda())
    assert (pred_reg - reg).abs().max().item() <= 1e-5 and (pred_cls - cls).abs().max().item() <= 1e-5
    m16 = make_model("vgg16", hp, B, precision="f16x3")
    m16.compile(learning_rate=lr)
    for _ in range(2):
        m16.train_on_batch(imgs, (deltas, labels))
    _, (reg16, cls16) = m16.test_on_batch(imgs, (deltas, labels), return_outputs=True)
    p_reg, p_cls = m16.predict_on_batch(torch.from_numpy(imgs).cuda())
    assert (p_reg - reg16).abs().max().item() <= 1e-4 and (p_cls - cls16).abs().max().item() <= 1e-4
    # fit: trainer.py:64-69's loop, one epoch of one step + one validation step
    hist = model.fit(iter([(imgs, (deltas, labels))]), steps_per_epoch=1, validation_data=iter([(imgs, (deltas, labels))]),
                     validation_steps=1)
    assert sorted(hist) == sorted(["loss", "rpn_reg_loss", "rpn_cls_loss", "val_loss", "val_rpn_reg_loss", "val_rpn_cls_loss"])
    assert np.isclose(hist["loss"][0], after[0], rtol=1e-6) and hist["val_loss"][0] < hist["loss"][0]
