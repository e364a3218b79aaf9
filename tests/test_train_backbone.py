"""Training of the VGG16 backbone (reference models/rpn_vgg16.py:16-21 + trainer.py:54-69: the Keras base model is trainable):
``compile(train_backbone_from=...)``, the 3x3 dgrad, the wide wgrad, the max-pool backward, and the whole-model step.

Oracles: float64 restatements (numpy / torch), torch float64 autograd of the full graph on the CPU.  Gradient forms as TF 2.0.0
computes them (restated from its sources as recalled -- nothing here can run TF): ReluGrad masks by the ReLU OUTPUT > 0; the CPU
MaxPoolGrad sends a window's gradient to its first maximum in row-major order (replaced only by a strictly greater value).
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
from tf_rpn_amd.models import rpn_vgg16  # noqa: E402
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, VGG16_CONVS, RPNModel, synthetic_weights  # noqa: E402
from tf_rpn_amd.utils import train_utils  # noqa: E402

EPS32 = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


def seeded_model(hp, B, from_layer, seed=3):
    """A VGG16 model compiled with train_backbone_from, its weights given to the Python side only (no device needed)."""
    m = RPNModel("vgg16", hp, max_batch=B)
    w = synthetic_weights("vgg16", hp, seed=seed)
    for name in HEAD_LAYERS:
        m._head[name] = (w[name]["kernel"], w[name]["bias"])
    for name in VGG16_CONVS:
        m._backbone[name] = (w[name]["kernel"], w[name]["bias"])
    m.compile(train_backbone_from=from_layer)
    return m, w


# ---- CPU: the Python surface and the ABI ----------------------------------------------------------------------------------
def test_compile_from_block4_returns_the_trained_span(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m, w = seeded_model(hp, 1, "block4_conv1")
    got = m.get_weights()
    want = set(HEAD_LAYERS) | {"block4_conv1", "block4_conv2", "block4_conv3", "block5_conv1", "block5_conv2", "block5_conv3"}
    assert set(got) == want
    for name in want:
        assert np.array_equal(got[name]["kernel"], w[name]["kernel"]) and np.array_equal(got[name]["bias"], w[name]["bias"]), name
    assert m.trained_layers()[0] == "block4_conv1"
    # a frozen conv has no gradient; the trainer says so before it looks for a step
    k = np.empty((3, 3, 256, 256), np.float32)
    b = np.empty((256,), np.float32)
    st = lib.rpn_head_trainer_get_gradient(m._t, b"block3_conv3", k.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p), None)
    assert st == L.RPN_ERR_INVALID and b"frozen" in lib.rpn_last_error()
    # ... but its constants come back
    assert lib.rpn_head_trainer_get_layer(m._t, b"block3_conv3", k.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p),
                                          None) == L.RPN_OK
    assert np.array_equal(k, w["block3_conv3"]["kernel"])
    # compiling again without train_backbone_from returns to the head-only trainer
    m.compile()
    assert set(m.get_weights()) == set(HEAD_LAYERS)


def test_compile_rejections(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m = RPNModel("vgg16", hp, max_batch=1)
    with pytest.raises(ValueError, match="not a VGG16 conv"):
        m.compile(train_backbone_from="block6_conv1")
    with pytest.raises(ValueError, match="not a VGG16 conv"):
        m.compile(train_backbone_from="rpn_conv")
    with pytest.raises(ValueError, match="frozen backbone") as e:
        m.compile(trainable=("rpn_conv", "rpn_cls", "rpn_reg", "block5_conv3"))
    assert "train_backbone_from" in str(e.value)
    with pytest.raises(ValueError, match="frozen backbone"):
        m.compile(trainable=("rpn_conv", "rpn_cls", "rpn_reg", "block5_conv3"), train_backbone_from="block5_conv3")
    hpm = bo.get_hyper_params("mobilenet_v2", img_size=224, feature_map_shape=14)
    mm = RPNModel("mobilenet_v2", hpm, max_batch=1)
    with pytest.raises(ValueError, match="head only"):
        mm.compile(train_backbone_from="block1_conv1")
    # the native constructor refuses the same things
    t = L.vp(0)
    assert lib.rpn_model_trainer_create(mm._h, b"block1_conv1", ctypes.byref(t)) == L.RPN_ERR_INVALID
    assert b"VGG16" in lib.rpn_last_error()
    assert lib.rpn_model_trainer_create(m._h, b"block9_conv9", ctypes.byref(t)) == L.RPN_ERR_INVALID
    assert lib.rpn_model_trainer_create(None, b"block1_conv1", ctypes.byref(t)) == L.RPN_ERR_INVALID
    # a head-only trainer still refuses backbone layers
    assert lib.rpn_model_trainer_create(m._h, None, ctypes.byref(t)) == L.RPN_OK
    k = np.zeros((3, 3, 512, 512), np.float32)
    b = np.zeros((512,), np.float32)
    st = lib.rpn_head_trainer_set_layer(t, b"block5_conv3", k.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p))
    assert st == L.RPN_ERR_INVALID and b"frozen" in lib.rpn_last_error()
    lib.rpn_head_trainer_destroy(t)


NEW_SYMBOLS = ("rpn_model_trainer_create", "rpn_conv3x3_dgrad_workspace_bytes", "rpn_conv3x3_dgrad_tile_n", "rpn_conv3x3_dgrad",
               "rpn_maxpool2x2_backward", "rpn_conv3x3_wgrad_wide_workspace_bytes", "rpn_conv3x3_wgrad_wide")


def test_backbone_entries_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in L.exported_symbols(), name
        assert hasattr(raw, name), name


def test_backbone_entries_validate_before_device_use(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, L.vp)
    need = lib.rpn_conv3x3_dgrad_workspace_bytes(8, 16)
    assert need >= 9 * 8 * 16 * 4 and lib.rpn_conv3x3_dgrad_workspace_bytes(0, 16) == 0
    ws = (ctypes.c_ubyte * need)()
    wsp = ctypes.cast(ws, L.vp)
    assert lib.rpn_conv3x3_dgrad(None, p, None, 1, 4, 4, 8, 16, p, wsp, need, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_dgrad(p, p, None, 1, 4, 4, 6, 16, p, wsp, need, None) == L.RPN_ERR_INVALID     # Cin % 4
    assert lib.rpn_conv3x3_dgrad(p, p, None, 1, 4, 4, 8, 24, p, wsp, need, None) == L.RPN_ERR_INVALID     # Cout % 16
    assert lib.rpn_conv3x3_dgrad(p, p, None, 0, 4, 4, 8, 16, p, wsp, need, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_dgrad(p, p, None, 1, 4, 4, 8, 16, p, wsp, need - 1, None) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_conv3x3_dgrad(p, p, None, 1, 4, 4, 8, 16, p, None, 0, None) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_maxpool2x2_backward(None, p, 1, 4, 4, 4, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_maxpool2x2_backward(p, p, 1, 1, 4, 4, p, None) == L.RPN_ERR_INVALID
    assert lib.rpn_maxpool2x2_backward(p, p, 1, 4, 4, 6, p, None) == L.RPN_ERR_INVALID
    needw = lib.rpn_conv3x3_wgrad_wide_workspace_bytes(1, 4, 4, 3, 64)
    assert needw > 0 and lib.rpn_conv3x3_wgrad_wide_workspace_bytes(1, 4, 4, 5, 64) == 0
    wsw = (ctypes.c_ubyte * needw)()
    wswp = ctypes.cast(wsw, L.vp)
    assert lib.rpn_conv3x3_wgrad_wide(p, p, 1, 4, 4, 3, 64, p, None, wswp, needw, None) == L.RPN_ERR_INVALID    # db required
    assert lib.rpn_conv3x3_wgrad_wide(p, None, 1, 4, 4, 3, 64, p, p, wswp, needw, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_wgrad_wide(p, p, 1, 4, 4, 6, 64, p, p, wswp, needw, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_wgrad_wide(p, p, 1, 4, 4, 3, 62, p, p, wswp, needw, None) == L.RPN_ERR_INVALID
    assert lib.rpn_conv3x3_wgrad_wide(p, p, 1, 4, 4, 3, 64, p, p, wswp, needw - 1, None) == L.RPN_ERR_WORKSPACE


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_backbone_entries_need_a_device(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, L.vp)
    need = lib.rpn_conv3x3_dgrad_workspace_bytes(8, 16)
    ws = (ctypes.c_ubyte * need)()
    assert lib.rpn_conv3x3_dgrad(p, p, p, 1, 2, 2, 8, 16, p, ctypes.cast(ws, L.vp), need, None) == L.RPN_ERR_NO_DEVICE
    assert lib.rpn_maxpool2x2_backward(p, p, 1, 2, 2, 4, p, None) == L.RPN_ERR_NO_DEVICE
    needw = lib.rpn_conv3x3_wgrad_wide_workspace_bytes(1, 2, 2, 4, 4)
    wsw = (ctypes.c_ubyte * needw)()
    assert lib.rpn_conv3x3_wgrad_wide(p, p, 1, 2, 2, 4, 4, p, p, ctypes.cast(wsw, L.vp), needw, None) == L.RPN_ERR_NO_DEVICE
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m, _ = seeded_model(hp, 1, "block1_conv1")
    assert lib.rpn_head_trainer_step(m._t, p, 1, p, p, 1, 1e-5, 0.9, 0.999, 1e-7, p, None) == L.RPN_ERR_NO_DEVICE


def test_backbone_kernel_budgets(lib):
    """No scratch; registers and LDS of the backbone backward kernels pinned.  dgrad<2> / wgrad (both instances of the one kernel,
    <true> with the row of ones behind db): four waves, 2 x 2 32x32 f32 accumulator blocks (64 registers) + staging, 40 KB of LDS
    (three workgroups per CU by LDS); dgrad<1>: 2 x 1 blocks, 32 KB."""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    budgets = {"conv3x3_dgrad_f32_kernel<2>": (128, 0, 40960), "conv3x3_dgrad_f32_kernel<1>": (96, 0, 32768),
               "conv3x3_wgrad_f32_kernel<true>": (128, 0, 40960), "conv3x3_wgrad_f32_kernel<false>": (128, 0, 40960),
               "maxpool2x2_backward_kernel": (48, 0, 0),
               "dgrad_weights_kernel": (40, 0, 0), "wgrad_tree_kernel": (16, 0, 0), "wgrad_wide_finish_kernel": (32, 0, 0),
               "pad_channels3to4_kernel": (16, 0, 0)}
    for name, (vgpr, sspill, lds) in budgets.items():
        assert name in tab, name
        v, ss, vs, scratch, lds_b, _wg = tab[name]
        assert v <= vgpr and ss <= sspill and vs == 0 and scratch == 0 and lds_b <= lds, (name, tab[name])


# ---- GPU: single layers --------------------------------------------------------------------------------------------------
def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def maxpool_backward64(y, dpool):
    """MaxPoolGrad (first maximum, row-major window order, strictly greater replaces) + ReluGrad of the pooled tensor."""
    B, H, W, C = y.shape
    OH, OW = H // 2, W // 2
    win = y[:, :2 * OH, :2 * OW].reshape(B, OH, 2, OW, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, OH, OW, 4, C)
    arg = np.argmax(win, axis=3)                    # numpy: the first occurrence of the maximum
    best = np.take_along_axis(win, arg[:, :, :, None], axis=3)[:, :, :, 0]
    g = np.where(best > 0, dpool, 0.0)
    out = np.zeros((B, OH, OW, 4, C))
    np.put_along_axis(out, arg[:, :, :, None], g[:, :, :, None], axis=3)
    dy = np.zeros((B, H, W, C))
    dy[:, :2 * OH, :2 * OW] = out.reshape(B, OH, OW, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * OH, 2 * OW, C)
    return dy


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,C", [(1, 500, 64), (3, 125, 64), (1, 125, 512), (3, 31, 512), (1, 31, 64)])
def test_maxpool_backward_bit_exact(lib, B, H, C):
    rng = np.random.RandomState(H + C + B)
    # small integers: many positive ties inside a window (the first-max rule), zeros (all-zero windows), negatives
    y = rng.randint(-1, 3, size=(B, H, H, C)).astype(np.float32)
    y[:, :8, :8] = 0.0                                                      # all-zero windows
    y[:, 8:10, 8:10] = 2.0                                                  # a window of four equal positive maxima
    dpool = rng.standard_normal((B, H // 2, H // 2, C)).astype(np.float32)
    out = torch.full((B, H, H, C), float("nan"), device="cuda")             # every entry must be written
    dy_, dp_ = cuda(y), cuda(dpool)
    L.check(lib.rpn_maxpool2x2_backward(L.ptr(dy_), L.ptr(dp_), B, H, H, C, L.ptr(out), L.stream_ptr()),
            "rpn_maxpool2x2_backward")
    got = out.cpu().numpy()
    ref = maxpool_backward64(y.astype(np.float64), dpool.astype(np.float64))
    assert np.array_equal(got, ref.astype(np.float32))
    if H % 2:
        assert not got[:, -1].any() and not got[:, :, -1].any()             # the uncovered row and column
    assert got[:, 8, 8].any() and not got[:, 8, 9].any() and not got[:, 9, 8].any()


def dgrad64(dy, w):
    """dx[b,y,x,ci] = sum_{r,s,co} dy[b,y+1-r,x+1-s,co] w[r,s,ci,co], float64."""
    B, H, W, _ = dy.shape
    dyp = np.zeros((B, H + 2, W + 2, dy.shape[3]))
    dyp[:, 1:H + 1, 1:W + 1] = dy
    dx = np.zeros((B, H, W, w.shape[2]))
    for r in range(3):
        for s in range(3):
            dx += dyp[:, 2 - r:2 - r + H, 2 - s:2 - s + W] @ w[r, s].T
    return dx


# (B, H, Cin, Cout, tile width the launcher picks): the 128-wide tile (conv3x3_dgrad_f32_kernel<2>) carries most of the dgrad time at
# batch 8, 500 x 500 (blocks 2-4); the 64-wide one (<1>) block 1, block 5 and small batches
DGRAD_SHAPES = [(1, 500, 64, 64, 64), (1, 62, 256, 512, 64), (2, 31, 512, 512, 64), (1, 15, 512, 512, 64), (3, 125, 128, 256, 64),
                (3, 125, 256, 256, 128), (1, 256, 128, 64, 128), (8, 62, 512, 512, 128)]


def test_dgrad_tile_choice(lib):
    for B, H, Cin, _Cout, tile in DGRAD_SHAPES:
        assert lib.rpn_conv3x3_dgrad_tile_n(B, H, H, Cin) == tile, (B, H, Cin)
    assert lib.rpn_conv3x3_dgrad_tile_n(8, 250, 250, 128) == 128          # block2_conv2 at the benchmarked batch
    assert lib.rpn_conv3x3_dgrad_tile_n(8, 31, 31, 512) == 64             # block 5
    assert lib.rpn_conv3x3_dgrad_tile_n(1, 8, 8, 2) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,Cin,Cout,tile", DGRAD_SHAPES)
def test_dgrad_integer_bit_exact(lib, B, H, Cin, Cout, tile):
    assert lib.rpn_conv3x3_dgrad_tile_n(B, H, H, Cin) == tile
    rng = np.random.RandomState(B * H + Cin)
    # |dy|, |w| <= 2: every partial sum stays below 4 * 9 * 512 < 2^24 -- exact in float32 whatever the order
    dy = rng.randint(-2, 3, size=(B, H, H, Cout)).astype(np.float32)
    w = rng.randint(-2, 3, size=(3, 3, Cin, Cout)).astype(np.float32)
    mask = rng.randint(-1, 2, size=(B, H, H, Cin)).astype(np.float32)
    ref = dgrad64(dy.astype(np.float64), w.astype(np.float64))
    need = lib.rpn_conv3x3_dgrad_workspace_bytes(Cin, Cout)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ddy, dw, dm = cuda(dy), cuda(w), cuda(mask)
    for use_mask in (False, True):
        out = torch.full((B, H, H, Cin), float("nan"), device="cuda")
        L.check(lib.rpn_conv3x3_dgrad(L.ptr(ddy), L.ptr(dw), L.ptr(dm) if use_mask else None, B, H, H, Cin, Cout, L.ptr(out),
                                      L.ptr(ws), need, L.stream_ptr()), "rpn_conv3x3_dgrad")
        want = np.where(mask > 0, ref, 0.0) if use_mask else ref
        assert np.array_equal(out.cpu().numpy(), want.astype(np.float32)), use_mask


def wgrad64(x, dy):
    B, H, W, Cin = x.shape
    xp = np.zeros((B, H + 2, W + 2, Cin))
    xp[:, 1:H + 1, 1:W + 1] = x
    d2 = dy.reshape(-1, dy.shape[3])
    dw = np.zeros((3, 3, Cin, dy.shape[3]))
    for r in range(3):
        for s in range(3):
            dw[r, s] = xp[:, r:r + H, s:s + W].reshape(-1, Cin).T @ d2
    return dw, d2.sum(0)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,Cin,Cout", [(2, 500, 3, 64), (1, 500, 64, 64), (2, 125, 128, 256)])
def test_wgrad_wide_integer_bit_exact(lib, B, H, Cin, Cout):
    rng = np.random.RandomState(B + H + Cin)
    # |x|, |dy| <= 2: |partial sums| <= 4 * 500 000 < 2^24
    x = rng.randint(-2, 3, size=(B, H, H, Cin)).astype(np.float32)
    dy = rng.randint(-2, 3, size=(B, H, H, Cout)).astype(np.float32)
    need = lib.rpn_conv3x3_wgrad_wide_workspace_bytes(B, H, H, Cin, Cout)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dx_, ddy = cuda(x), cuda(dy)
    runs = []
    for _ in range(2):
        dw = torch.full((3, 3, Cin, Cout), float("nan"), device="cuda")
        db = torch.full((Cout,), float("nan"), device="cuda")
        L.check(lib.rpn_conv3x3_wgrad_wide(L.ptr(dx_), L.ptr(ddy), B, H, H, Cin, Cout, L.ptr(dw), L.ptr(db), L.ptr(ws), need,
                                           L.stream_ptr()), "rpn_conv3x3_wgrad_wide")
        runs.append((dw.cpu().numpy(), db.cpu().numpy()))
    ref_w, ref_b = wgrad64(x.astype(np.float64), dy.astype(np.float64))
    assert np.array_equal(runs[0][0], ref_w.astype(np.float32))
    assert np.array_equal(runs[0][1], ref_b.astype(np.float32))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


# ---- GPU: the whole model ---------------------------------------------------------------------------------------------------
HP250 = dict(img_size=250, feature_map_shape=15)            # odd pools: 125 -> 62, 31 -> 15


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


def batch(hp, B, seed):
    rng = np.random.RandomState(seed)
    imgs = rng.uniform(0, 1, size=(B, hp["img_size"], hp["img_size"], 3)).astype(np.float32)
    deltas, labels = targets(hp, B, seed)
    return imgs, deltas, labels


def make_model(hp, B, precision="f32", seed=1):
    model, _ = rpn_vgg16.get_model(hp, precision=precision, max_batch=B, seed=seed)
    return model


def full64(imgs, wts, deltas, labels):
    """VGG16 + RPN head + both losses in torch float64; returns (leaf params, reg loss, cls loss)."""
    F = torch.nn.functional
    params = {n: [torch.tensor(np.asarray(wts[n]["kernel"], np.float64), requires_grad=True),
                  torch.tensor(np.asarray(wts[n]["bias"], np.float64), requires_grad=True)] for n in VGG16_CONVS + HEAD_LAYERS}
    x = torch.tensor(np.asarray(imgs, np.float64)).permute(0, 3, 1, 2)
    for n in VGG16_CONVS:
        k, b = params[n]
        x = torch.relu(F.conv2d(x, k.permute(3, 2, 0, 1), b, padding=1))
        if n in ("block1_conv2", "block2_conv2", "block3_conv3", "block4_conv3"):
            x = F.max_pool2d(x, 2, 2)
    k, b = params["rpn_conv"]
    s = torch.relu(F.conv2d(x, k.permute(3, 2, 0, 1), b, padding=1)).permute(0, 2, 3, 1)
    reg = s @ params["rpn_reg"][0][0, 0] + params["rpn_reg"][1]
    cls = torch.sigmoid(s @ params["rpn_cls"][0][0, 0] + params["rpn_cls"][1])
    yt = torch.tensor(deltas, dtype=torch.float64)
    a = (reg.reshape(reg.shape[0], -1, 4) - yt).abs()
    q = torch.clamp(a, max=1.0)
    pos = (yt != 0).any(-1).to(torch.float64)
    r = (pos * (0.5 * q * q + (a - q)).sum(-1)).sum() / torch.clamp(pos.sum(), min=1.0)
    lt = torch.tensor(labels, dtype=torch.float64)
    keep = lt != -1
    pc = torch.clamp(cls[keep], EPS32, CLIP_HI)
    c = -(lt[keep] * torch.log(pc + EPS32) + (1 - lt[keep]) * torch.log(1 - pc + EPS32)).mean()
    return params, r, c


@pytest.mark.gpu
def test_whole_model_gradients_match_float64_autograd(lib):
    hp = bo.get_hyper_params("vgg16", **HP250)
    B = 2
    model = make_model(hp, B)
    w0 = synthetic_weights("vgg16", hp, seed=1)
    imgs, deltas, labels = batch(hp, B, seed=61)
    model.compile(train_backbone_from="block1_conv1")
    losses = model.train_on_batch(imgs, (deltas, labels))
    grads = model.get_gradients()
    assert set(grads) == set(VGG16_CONVS + HEAD_LAYERS)
    params, r, c = full64(imgs, w0, deltas, labels)
    (r + c).backward()
    assert np.allclose(losses, [(r + c).item(), r.item(), c.item()], rtol=1e-5, atol=0)
    # Above block4_pool (block5_* and the head) the error is float32 rounding: measured at most 1.3e-6 of max|g64| (rpn_reg's
    # kernel), bounded at 5e-6.  From block4_conv3 down it is dominated by max-pool windows whose two largest entries differ by less
    # than the float32 forward's rounding: the float32 and float64 forwards pick different maxima and route that window's gradient
    # to different pixels.  torch float32 autograd of the same graph on the CPU shows the same: 2.4e-3 of max|g64| at block4_conv3
    # against this step's 3.0e-3 (measured worst, block4_conv3's kernel; block1_conv1: 2.6e-3 against torch's 1.1e-3); bounded
    # at 5e-3.  The single-layer kernels are bit-exact (the tests above), and so is the truncated backward.
    for name in VGG16_CONVS + HEAD_LAYERS:
        bound = 5e-6 if name.startswith("block5") or name in HEAD_LAYERS else 5e-3
        for i, key in enumerate(("kernel", "bias")):
            g64 = params[name][i].grad.numpy()
            rel = np.abs(grads[name][key] - g64).max() / np.abs(g64).max()
            assert rel <= bound, (name, key, rel)


@pytest.mark.gpu
def test_truncated_backward_gives_the_same_bits(lib):
    hp = bo.get_hyper_params("vgg16", **HP250)
    B = 2
    model = make_model(hp, B)
    w0 = synthetic_weights("vgg16", hp, seed=1)
    imgs, deltas, labels = batch(hp, B, seed=62)
    model.compile(train_backbone_from="block1_conv1")
    l_full = model.train_on_batch(imgs, (deltas, labels))
    g_full = model.get_gradients()
    model.set_weights(w0)                   # back to the seeded weights (the handle's and the trainer's)
    model.compile(train_backbone_from="block4_conv1")
    l_part = model.train_on_batch(imgs, (deltas, labels))
    g_part = model.get_gradients()
    assert l_full == l_part
    assert set(g_part) == set(VGG16_CONVS[7:] + HEAD_LAYERS)
    for name in g_part:
        for key in ("kernel", "bias"):
            assert g_part[name][key].tobytes() == g_full[name][key].tobytes(), (name, key)
    for _ in range(2):
        model.train_on_batch(imgs, (deltas, labels))
    for name in VGG16_CONVS[:7]:            # frozen: bit-unchanged
        k = np.empty(w0[name]["kernel"].shape, np.float32)
        b = np.empty(w0[name]["bias"].shape, np.float32)
        L.check(lib.rpn_head_trainer_get_layer(model._t, name.encode(), k.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p),
                                               L.stream_ptr()), "get_layer")
        assert k.tobytes() == w0[name]["kernel"].tobytes() and b.tobytes() == w0[name]["bias"].tobytes(), name
    assert set(model.get_weights()) == set(g_part)


def adam64(w, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-7):
    alpha = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    m = m + (g - m) * (1 - b1)
    v = v + (g * g - v) * (1 - b2)
    return w - alpha * m / (np.sqrt(v) + eps), m, v


@pytest.mark.gpu
def test_adam_on_the_extended_buffer(lib):
    hp = bo.get_hyper_params("vgg16", **HP250)
    model = make_model(hp, 2)
    imgs, deltas, labels = batch(hp, 2, seed=63)
    lr = 1e-4
    model.compile(learning_rate=lr, train_backbone_from="block1_conv1")
    w64 = {n: {k: v.astype(np.float64) for k, v in d.items()} for n, d in model.get_weights().items()}
    assert set(w64) == set(VGG16_CONVS + HEAD_LAYERS)
    mv = {n: {k: (np.zeros_like(v), np.zeros_like(v)) for k, v in d.items()} for n, d in w64.items()}
    for t in (1, 2, 3):
        model.train_on_batch(imgs, (deltas, labels))
        g = model.get_gradients()
        for n in w64:
            for k in ("kernel", "bias"):
                w64[n][k], m, v = adam64(w64[n][k], g[n][k].astype(np.float64), *mv[n][k], t, lr)
                mv[n][k] = (m, v)
        got = model.get_weights()
        for n in w64:
            for k in ("kernel", "bias"):
                ref = w64[n][k]
                assert np.abs(got[n][k] - ref).max() <= 1e-6 * np.abs(ref).max(), (t, n, k)
        model.test_on_batch(imgs, (deltas, labels))
        assert model.train_steps() == t
        after = model.get_weights()
        assert all(after[n]["kernel"].tobytes() == got[n]["kernel"].tobytes() for n in w64)


@pytest.mark.gpu
def test_backbone_step_is_deterministic(lib):
    hp = bo.get_hyper_params("vgg16")
    model = make_model(hp, 8)
    w0 = synthetic_weights("vgg16", hp, seed=1)
    imgs, deltas, labels = batch(hp, 8, seed=64)
    runs = []
    for _ in range(2):
        model.set_weights(w0)
        model.compile(train_backbone_from="block1_conv1")
        losses = model.train_on_batch(imgs, (deltas, labels))
        runs.append((losses, model.get_weights()))
    assert runs[0][0] == runs[1][0]
    assert set(runs[0][1]) == set(VGG16_CONVS + HEAD_LAYERS)
    for n in runs[0][1]:
        for k in ("kernel", "bias"):
            assert runs[0][1][n][k].tobytes() == runs[1][1][n][k].tobytes(), (n, k)


@pytest.mark.gpu
def test_inference_after_backbone_training(lib, tmp_path):
    hp = bo.get_hyper_params("vgg16", **HP250)
    B, lr = 2, 1e-4
    imgs, deltas, labels = batch(hp, B, seed=65)
    x = torch.from_numpy(imgs).cuda()
    model = make_model(hp, B)
    model.compile(learning_rate=lr, train_backbone_from="block1_conv1")
    for _ in range(2):
        model.train_on_batch(imgs, (deltas, labels))
    _, (reg, cls) = model.test_on_batch(imgs, (deltas, labels), return_outputs=True)
    p_reg, p_cls = model.predict_on_batch(x)
    assert (p_reg - reg).abs().max().item() <= 1e-5 and (p_cls - cls).abs().max().item() <= 1e-5
    # the f16x3 handle repacks every trained layer (block 1 as its fused op)
    m16 = make_model(hp, B, precision="f16x3")
    m16.compile(learning_rate=lr, train_backbone_from="block1_conv1")
    for _ in range(2):
        m16.train_on_batch(imgs, (deltas, labels))
    _, (reg16, cls16) = m16.test_on_batch(imgs, (deltas, labels), return_outputs=True)
    q_reg, q_cls = m16.predict_on_batch(x)
    assert (q_reg - reg16).abs().max().item() <= 1e-4 and (q_cls - cls16).abs().max().item() <= 1e-4
    # save_weights -> load_weights into a fresh model reproduces the predictions
    path = str(tmp_path / "trained.npz")
    RPNModel.save_weights(model.get_weights(), path)
    fresh = make_model(hp, B)
    assert set(fresh.load_weights(path)) == set(VGG16_CONVS + HEAD_LAYERS)
    f_reg, f_cls = fresh.predict_on_batch(x)
    assert torch.equal(f_reg, p_reg) and torch.equal(f_cls, p_cls)


@pytest.mark.gpu
def test_fit_from_block1_reduces_the_loss(lib):
    hp = bo.get_hyper_params("vgg16", **HP250)
    imgs, deltas, labels = batch(hp, 2, seed=66)
    model = make_model(hp, 2)
    model.compile(learning_rate=1e-4, train_backbone_from="block1_conv1")
    before = model.test_on_batch(imgs, (deltas, labels))[0]
    gen = iter([(imgs, (deltas, labels))] * 5)
    hist = model.fit(gen, steps_per_epoch=5)
    after = model.test_on_batch(imgs, (deltas, labels))[0]
    assert np.isfinite(hist["loss"][0]) and after < before, (before, after)
