"""Joint training: the backbone trained with the RPN's gradient plus a second stage's gradient at the feature tap.

``rpn_conv3x3_dgrad_add`` (the addend in the 3x3 dgrad's epilogue), the training step in two halves (``rpn_head_trainer_forward`` /
``_feature`` / ``_backward``) and ``RPNModel.forward_for_training`` / ``apply_gradients`` / ``train_on_batch(second_stage=...)``.

Oracles: float64 restatements (numpy), torch float64 autograd of the whole graph on the CPU with ``L2 = sum(G * feat)`` added, and the
plain step itself (the split must reproduce its bytes).  Helpers, shapes and the float64 graphs come from test_train_backbone.py,
test_train_mobilenet.py and test_train_mobilenet_full.py.
"""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402
import test_train_backbone as vb  # noqa: E402
import test_train_mobilenet as ms  # noqa: E402
import test_train_mobilenet_full as mf  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from test_train_mobilenet import span_case  # noqa: E402,F401  (fixture)
from test_train_mobilenet_full import full_case  # noqa: E402,F401  (fixture)
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.models._rpn_model import HEAD_LAYERS, VGG16_CONVS, RPNModel, synthetic_weights  # noqa: E402
from tf_rpn_amd.utils.roi_utils import roi_pooling, roi_pooling_backward  # noqa: E402

TF = torch.nn.functional
NEW_SYMBOLS = ("rpn_conv3x3_dgrad_add", "rpn_head_trainer_forward", "rpn_head_trainer_feature", "rpn_head_trainer_backward")
ADAM = (1e-5, 0.9, 0.999, 1e-7)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


# ---- CPU: the ABI and the Python surface ----------------------------------------------------------------------------------------
def test_joint_entries_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in L.exported_symbols(), name
        assert hasattr(raw, name), name
    assert lib.rpn_abi_version() == 1


def test_dgrad_add_validates_before_device_use(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, L.vp)
    need = lib.rpn_conv3x3_dgrad_workspace_bytes(8, 16)
    ws = (ctypes.c_ubyte * need)()
    wsp = ctypes.cast(ws, L.vp)
    call = lib.rpn_conv3x3_dgrad_add
    for args in ((None, p, p, p), (p, None, p, p), (p, p, p, None)):            # dy, w, add: required (the mask is optional)
        assert call(*args, 1, 4, 4, 8, 16, p, wsp, need, None) == L.RPN_ERR_INVALID
        assert b"null pointer" in lib.rpn_last_error()
    assert call(p, p, None, p, 1, 4, 4, 8, 16, None, wsp, need, None) == L.RPN_ERR_INVALID
    assert call(p, p, None, L.vp(p.value + 2), 1, 4, 4, 8, 16, p, wsp, need, None) == L.RPN_ERR_INVALID
    assert b"4-byte aligned" in lib.rpn_last_error()
    assert call(p, p, None, p, 1, 4, 4, 6, 16, p, wsp, need, None) == L.RPN_ERR_INVALID      # Cin % 4
    assert call(p, p, None, p, 1, 4, 4, 8, 24, p, wsp, need, None) == L.RPN_ERR_INVALID      # Cout % 16
    assert call(p, p, None, p, 0, 4, 4, 8, 16, p, wsp, need, None) == L.RPN_ERR_INVALID
    assert call(p, p, None, p, 1, 4, 4, 8, 16, p, wsp, need - 1, None) == L.RPN_ERR_WORKSPACE
    assert call(p, p, None, p, 1, 4, 4, 8, 16, p, None, 0, None) == L.RPN_ERR_WORKSPACE


def test_dgrad_tile_choice_is_unchanged(lib):
    for B, H, Cin, _Cout, tile in vb.DGRAD_SHAPES:
        assert lib.rpn_conv3x3_dgrad_tile_n(B, H, H, Cin) == tile, (B, H, Cin)
    # the rule itself: 128 x 128 tiles only when they still give two per CU of 256
    for B, H, Cin in ((1, 15, 512), (2, 7, 68), (1, 5, 4), (8, 31, 512), (8, 250, 128), (1, 256, 128), (4, 128, 128), (4, 127, 128)):
        mt = (B * H * H + 127) // 128
        want = 128 if Cin >= 128 and mt * ((Cin + 127) // 128) >= 512 else 64
        assert lib.rpn_conv3x3_dgrad_tile_n(B, H, H, Cin) == want, (B, H, Cin)
    assert lib.rpn_conv3x3_dgrad_tile_n(1, 8, 8, 2) == 0


def test_two_halves_validate_before_device_use(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, L.vp)
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m, _ = vb.seeded_model(hp, 2, "block4_conv1")
    t = m._t
    fwd, bwd, feat = lib.rpn_head_trainer_forward, lib.rpn_head_trainer_backward, lib.rpn_head_trainer_feature
    for args in ((None, p, 1, p, p), (t, None, 1, p, p), (t, p, 1, None, p), (t, p, 1, p, None)):
        assert fwd(*args, 1, p, None) == L.RPN_ERR_INVALID
    assert fwd(t, p, 1, p, p, 1, None, None) == L.RPN_ERR_INVALID
    assert fwd(t, p, 3, p, p, 1, p, None) == L.RPN_ERR_INVALID                   # batch > max_batch
    for train in (2, -1):
        assert fwd(t, p, 1, p, p, train, p, None) == L.RPN_ERR_INVALID
        assert b"train must be 0 or 1" in lib.rpn_last_error()
    assert bwd(None, p, 1, None, *ADAM, None) == L.RPN_ERR_INVALID
    assert bwd(t, None, 1, None, *ADAM, None) == L.RPN_ERR_INVALID
    assert bwd(t, p, 1, None, 1e-5, 1.5, 0.999, 1e-7, None) == L.RPN_ERR_INVALID  # beta_1 >= 1
    assert b"Adam" in lib.rpn_last_error()
    assert bwd(t, p, 1, None, float("nan"), 0.9, 0.999, 1e-7, None) == L.RPN_ERR_INVALID
    assert bwd(t, p, 1, None, 1e-5, 0.9, 0.999, -1.0, None) == L.RPN_ERR_INVALID
    assert bwd(t, p, 1, None, *ADAM, None) == L.RPN_ERR_INVALID
    assert b"no pending" in lib.rpn_last_error()
    assert bwd(t, p, 1, p, *ADAM, None) == L.RPN_ERR_INVALID and b"no pending" in lib.rpn_last_error()
    assert feat(None, p, 1, None) == L.RPN_ERR_INVALID and feat(t, None, 1, None) == L.RPN_ERR_INVALID
    assert feat(t, p, 1, None) == L.RPN_ERR_INVALID                              # no forward has run
    assert lib.rpn_head_trainer_steps(t) == 0
    # a trainer whose head was never set
    t2 = L.vp(0)
    assert lib.rpn_head_trainer_create(m._h, ctypes.byref(t2)) == L.RPN_OK
    assert fwd(t2, p, 1, p, p, 1, p, None) == L.RPN_ERR_INVALID and b"never set" in lib.rpn_last_error()
    # a frozen backbone refuses a feature gradient, and says why, before it looks for a pending forward
    assert bwd(t2, p, 1, p, *ADAM, None) == L.RPN_ERR_INVALID
    assert b"frozen backbone" in lib.rpn_last_error() and b"nothing below the feature tap trains" in lib.rpn_last_error()
    assert bwd(t2, p, 1, None, *ADAM, None) == L.RPN_ERR_INVALID and b"no pending" in lib.rpn_last_error()
    lib.rpn_head_trainer_destroy(t2)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_joint_entries_need_a_device(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, L.vp)
    need = lib.rpn_conv3x3_dgrad_workspace_bytes(8, 16)
    ws = (ctypes.c_ubyte * need)()
    assert lib.rpn_conv3x3_dgrad_add(p, p, p, p, 1, 2, 2, 8, 16, p, ctypes.cast(ws, L.vp), need, None) == L.RPN_ERR_NO_DEVICE
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m, _ = vb.seeded_model(hp, 1, "block1_conv1")
    for train in (0, 1):
        assert lib.rpn_head_trainer_forward(m._t, p, 1, p, p, train, p, None) == L.RPN_ERR_NO_DEVICE
    # nothing became pending
    assert lib.rpn_head_trainer_backward(m._t, p, 1, None, *ADAM, None) == L.RPN_ERR_INVALID
    assert lib.rpn_head_trainer_feature(m._t, p, 1, None) == L.RPN_ERR_INVALID


def test_python_refusals_without_a_device(lib):
    hp = bo.get_hyper_params("vgg16", img_size=224, feature_map_shape=14)
    m, _ = vb.seeded_model(hp, 2, "block4_conv1")
    for bad in (torch.zeros(1, 14, 14, 256), torch.zeros(1, 14, 13, 512), torch.zeros(14, 14, 512), torch.zeros(3, 14, 14, 512)):
        with pytest.raises(ValueError, match="feature_grad must be"):
            m.apply_gradients(bad)
    with pytest.raises(ValueError, match="float32"):
        m.apply_gradients(torch.zeros(1, 14, 14, 512, dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA tensor, got torch.float32 on cpu"):
        m.apply_gradients(torch.zeros(1, 14, 14, 512))
    with pytest.raises(ValueError, match="contiguous"):
        m.apply_gradients(torch.zeros(1, 14, 512, 14).permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="torch tensor"):
        m.apply_gradients(np.zeros((1, 14, 14, 512), np.float32))
    with pytest.raises(RuntimeError, match="pending"):
        m.apply_gradients()
    m.compile()                                                                  # the head only: a frozen backbone
    with pytest.raises(ValueError, match="frozen backbone") as e:
        m.train_on_batch(np.zeros((1, 224, 224, 3), np.float32), (None, None), second_stage=lambda feat, reg, cls: feat.sum())
    assert "train_backbone_from" in str(e.value)
    with pytest.raises(ValueError, match="nothing below the feature tap trains") as e:
        m.apply_gradients(torch.zeros(1, 14, 14, 512))                           # refused before anything else is looked at
    assert "frozen backbone" in str(e.value) and "train_backbone_from" in str(e.value)
    mm, _ = ms.seeded_model(ms.hp_for(80), 1, "block_12_expand")
    with pytest.raises(ValueError, match="feature_grad must be"):
        mm.apply_gradients(torch.zeros(1, 5, 5, 512))                            # MobileNetV2's tap has 576 channels


def test_dgrad_add_kernel_budgets(lib):
    """The addend's kernels are held to the plain dgrad kernels' budgets (test_train_backbone.test_backbone_kernel_budgets): four waves
    per SIMD on the 128-wide tile (<= 128 registers), no scratch, the same LDS.  Built: 102 and 65 registers."""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    for name, (vgpr, lds) in {"conv3x3_dgrad_add_f32_kernel<2>": (128, 40960), "conv3x3_dgrad_add_f32_kernel<1>": (96, 32768)}.items():
        assert name in tab, name
        v, ss, vs, scratch, lds_b, _wg = tab[name]
        assert v <= vgpr and ss == 0 and vs == 0 and scratch == 0 and lds_b <= lds, (name, tab[name])


# ---- GPU 1: the epilogue, bit-exact -----------------------------------------------------------------------------------------------
# (B, H, Cin, Cout, tile): the 64-wide tile whole, with a partial channel tile (Cin % 64 != 0, two pixel blocks would need 128 pixels:
# 98 here, one partial block), with a partial pixel tile; the 128-wide tile
ADD_SHAPES = [(1, 15, 512, 512, 64), (2, 7, 68, 16, 64), (1, 5, 4, 16, 64), (1, 256, 128, 64, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,Cin,Cout,tile", ADD_SHAPES)
def test_dgrad_add_integer_bit_exact(lib, B, H, Cin, Cout, tile):
    assert lib.rpn_conv3x3_dgrad_tile_n(B, H, H, Cin) == tile
    rng = np.random.RandomState(B * H + Cin + 1)
    # |dy|, |w| <= 2, |add| <= 3: every partial sum stays below 4 * 9 * 512 + 3 < 2^24 -- exact in float32 whatever the order
    dy = rng.randint(-2, 3, size=(B, H, H, Cout)).astype(np.float32)
    w = rng.randint(-2, 3, size=(3, 3, Cin, Cout)).astype(np.float32)
    add = rng.randint(-3, 4, size=(B, H, H, Cin)).astype(np.float32)
    mask = rng.randint(-1, 2, size=(B, H, H, Cin)).astype(np.float32)
    ref = vb.dgrad64(dy.astype(np.float64), w.astype(np.float64))
    need = lib.rpn_conv3x3_dgrad_workspace_bytes(Cin, Cout)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ddy, dw, dm, da = vb.cuda(dy), vb.cuda(w), vb.cuda(mask), vb.cuda(add)
    zeros = torch.zeros_like(da)

    def run(mask_t, add_t, out=None):
        out = torch.full((B, H, H, Cin), float("nan"), device="cuda") if out is None else out
        add_p = L.ptr(out) if add_t is out else L.ptr(add_t)
        if add_t is None:
            L.check(lib.rpn_conv3x3_dgrad(L.ptr(ddy), L.ptr(dw), L.ptr(mask_t), B, H, H, Cin, Cout, L.ptr(out), L.ptr(ws), need,
                                          L.stream_ptr()), "rpn_conv3x3_dgrad")
        else:
            L.check(lib.rpn_conv3x3_dgrad_add(L.ptr(ddy), L.ptr(dw), L.ptr(mask_t), add_p, B, H, H, Cin, Cout, L.ptr(out), L.ptr(ws),
                                              need, L.stream_ptr()), "rpn_conv3x3_dgrad_add")
        return out.cpu().numpy()

    for mask_t in (None, dm):
        want = (np.where(mask > 0, ref + add, 0.0) if mask_t is not None else ref + add).astype(np.float32)
        assert np.array_equal(run(mask_t, da), want), mask_t is not None
        assert run(mask_t, zeros).tobytes() == run(mask_t, None).tobytes()       # add = 0: the plain kernel's bytes
    if (B, H, Cin) in ((2, 7, 68), (1, 256, 128)):                               # in place, once per tile width
        out = da.clone()
        assert np.array_equal(run(dm, out, out=out), np.where(mask > 0, ref + add, 0.0).astype(np.float32))


# ---- GPU: VGG16 at HP250, batch 2 ---------------------------------------------------------------------------------------------------
def state(model):
    return {(n, k): v.tobytes() for n, d in model.get_weights().items() for k, v in d.items()}


def grad_bytes(model):
    return {(n, k): v.tobytes() for n, d in model.get_gradients().items() for k, v in d.items()}


def step(model, batch, kind, G=None):
    """One update on a freshly compiled model -> (losses as bytes, gradient bytes, weight bytes).  kind: "plain" (train_on_batch) or
    "split" (forward_for_training + apply_gradients(G))."""
    imgs, deltas, labels = batch
    if kind == "plain":
        losses = np.asarray(model.train_on_batch(imgs, (deltas, labels)), np.float32)
    else:
        l, feat, (reg, cls) = model.forward_for_training(imgs, (deltas, labels))
        assert feat.dtype == torch.float32 and feat.is_cuda and tuple(l.shape) == (3,)
        model.apply_gradients(G)
        losses = l.cpu().numpy()
    return losses.tobytes(), grad_bytes(model), state(model)


def vgg_graph(imgs, wts, deltas, labels, dtype):
    """test_train_backbone.full64 with the dtype a parameter -> (leaf params, reg loss, cls loss, the tap (B,F,F,512) in the graph)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)
    params = {n: [t(wts[n]["kernel"]).requires_grad_(True), t(wts[n]["bias"]).requires_grad_(True)] for n in VGG16_CONVS + HEAD_LAYERS}
    x = t(imgs).permute(0, 3, 1, 2)
    for n in VGG16_CONVS:
        k, b = params[n]
        x = torch.relu(TF.conv2d(x, k.permute(3, 2, 0, 1), b, padding=1))
        if n in ("block1_conv2", "block2_conv2", "block3_conv3", "block4_conv3"):
            x = TF.max_pool2d(x, 2, 2)
    feat = x.permute(0, 2, 3, 1)
    k, b = params["rpn_conv"]
    s = torch.relu(TF.conv2d(feat.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), b, padding=1)).permute(0, 2, 3, 1)
    reg = s @ params["rpn_reg"][0][0, 0] + params["rpn_reg"][1]
    cls = torch.sigmoid(s @ params["rpn_cls"][0][0, 0] + params["rpn_cls"][1])
    yt = t(deltas)
    a = (reg.reshape(reg.shape[0], -1, 4) - yt).abs()
    q = torch.clamp(a, max=1.0)
    pos = (yt != 0).any(-1).to(dtype)
    r = (pos * (0.5 * q * q + (a - q)).sum(-1)).sum() / torch.clamp(pos.sum(), min=1.0)
    lt = t(labels)
    keep = lt != -1
    pc = torch.clamp(cls[keep], vb.EPS32, vb.CLIP_HI)
    c = -(lt[keep] * torch.log(pc + vb.EPS32) + (1 - lt[keep]) * torch.log(1 - pc + vb.EPS32)).mean()
    return params, r, c, feat


def seeded_G(shape, scale, seed=5):
    """The fixed second-stage gradient: seeded normal values scaled to the RPN's own mean |gradient| at the tap."""
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


@pytest.fixture(scope="module")
def vgg_case(lib):
    """One model, one batch; the float64 and float32 torch runs of r + c + sum(G * feat); the plain step and the joint step with G from
    block1_conv1, each run once and shared."""
    hp = bo.get_hyper_params("vgg16", **vb.HP250)
    B = 2
    w0 = synthetic_weights("vgg16", hp, seed=1)
    batch = vb.batch(hp, B, seed=61)
    p64, r, c, feat = vgg_graph(*batch[:1], w0, *batch[1:], torch.float64)
    g_rpn, = torch.autograd.grad(r + c, feat, retain_graph=True)
    G = seeded_G(tuple(feat.shape), float(g_rpn.abs().mean()))
    (r + c + (torch.tensor(G.astype(np.float64)) * feat).sum()).backward()
    p32, r32, c32, feat32 = vgg_graph(*batch[:1], w0, *batch[1:], torch.float32)
    (r32 + c32 + (torch.tensor(G) * feat32).sum()).backward()
    model = vb.make_model(hp, B)
    case = dict(hp=hp, B=B, w0=w0, batch=batch, model=model, G=G, Gd=torch.from_numpy(G).cuda(), p64=p64, p32=p32,
                g_rpn_mean=float(g_rpn.abs().mean()), g_rpn_max=float(g_rpn.abs().max()))
    case["plain"] = step(fresh_vgg(case), batch, "plain")
    case["joint"] = step(fresh_vgg(case), batch, "split", case["Gd"])
    case["joint_grads"] = model.get_gradients()
    return case


def fresh_vgg(case, first="block1_conv1", **kw):
    m = case["model"]
    m.set_weights(case["w0"])                   # back to the seeded weights (the handle's and the trainer's)
    m.compile(train_backbone_from=first, **kw)
    return m


@pytest.mark.gpu
def test_split_is_the_step_vgg16(lib, vgg_case):
    case = vgg_case
    assert step(fresh_vgg(case), case["batch"], "split", None) == case["plain"]
    assert step(fresh_vgg(case), case["batch"], "split", torch.zeros_like(case["Gd"])) == case["plain"]
    assert set(k[0] for k in case["plain"][1]) == set(VGG16_CONVS + HEAD_LAYERS)


@pytest.mark.gpu
def test_split_is_the_step_mobilenet_whole(lib, full_case):
    case = full_case
    batch = (case["imgs"], case["deltas"], case["labels"])
    plain = step(mf.fresh(case), batch, "plain")
    assert step(mf.fresh(case), batch, "split", None) == plain
    assert step(mf.fresh(case), batch, "split", torch.zeros((mf.BATCH, 3, 3, 576), device="cuda")) == plain
    assert len(plain[1]) == 40 * 3 + 6 and (mf.bn_of("Conv1"), "mean") in plain[2]     # the moving statistics are compared too


@pytest.mark.gpu
def test_split_is_the_step_mobilenet_span(lib, span_case):
    case = span_case
    batch = (case["imgs"], case["deltas"], case["labels"])
    F = case["model"].feature_map_shape
    plain = step(ms.fresh(case, "block_7_expand"), batch, "plain")
    assert step(ms.fresh(case, "block_7_expand"), batch, "split", None) == plain
    assert step(ms.fresh(case, "block_7_expand"), batch, "split", torch.zeros((ms.BATCH, F, F, 576), device="cuda")) == plain
    assert ("block_7_expand", "kernel") in plain[1] and ("block_6_project", "kernel") not in plain[1]


@pytest.mark.gpu
def test_split_is_the_step_on_a_frozen_backbone(lib):
    """A head-only compile: the two halves give train_on_batch's bytes, a feature gradient is refused with the forward still pending,
    and rpn_head_trainer_feature returns the handle's tap as the head trainer read it (d_feat)."""
    hp = bo.get_hyper_params("vgg16", img_size=96, feature_map_shape=6)
    B = 2
    w0 = synthetic_weights("vgg16", hp, seed=1)
    batch = vb.batch(hp, B, seed=67)
    m = RPNModel("vgg16", hp, precision="f32", max_batch=B, keep_activations=True)
    runs = []
    for kind in ("plain", "split"):
        m.set_weights(w0)
        m.compile()
        runs.append(step(m, batch, kind, None))
    assert runs[0] == runs[1] and set(k[0] for k in runs[0][1]) == set(HEAD_LAYERS)
    m.set_weights(w0)
    m.compile()
    x = torch.from_numpy(batch[0]).cuda()
    _, feat, _ = m.forward_for_training(x, batch[1:])
    with pytest.raises(ValueError, match="frozen backbone"):
        m.apply_gradients(torch.zeros_like(feat))
    assert lib.rpn_head_trainer_backward(m._t, L.ptr(x), B, L.ptr(feat), *ADAM, L.stream_ptr()) == L.RPN_ERR_INVALID
    assert b"nothing below the feature tap trains" in lib.rpn_last_error()
    m.apply_gradients(None)                                                      # the refusals consumed nothing
    assert m.train_steps() == 1
    m.set_weights(w0)
    m.predict_on_batch(x)
    assert torch.equal(feat, m.get_activation("block5_conv3", batch=B))          # the float32 handle's tap, bit for bit


# ---- GPU 3: the head's gradients do not depend on the addend ------------------------------------------------------------------------
@pytest.mark.gpu
def test_head_gradients_are_independent_of_the_addend_vgg16(lib, vgg_case):
    plain, joint = vgg_case["plain"][1], vgg_case["joint"][1]
    for name in HEAD_LAYERS:
        for key in ("kernel", "bias"):
            assert joint[(name, key)] == plain[(name, key)], (name, key)
    assert joint[("block5_conv3", "kernel")] != plain[("block5_conv3", "kernel")]
    assert joint[("block5_conv3", "bias")] != plain[("block5_conv3", "bias")]
    assert joint[("block1_conv1", "kernel")] != plain[("block1_conv1", "kernel")]          # ... and it reaches the bottom
    assert vgg_case["joint"][0] == vgg_case["plain"][0]                                    # the RPN's losses are the forward's


@pytest.fixture(scope="module")
def mn_joint(lib, full_case):
    """Whole MobileNetV2: the float64 / float32 torch runs of r + c + sum(G * feat) on test_train_mobilenet_full's graph (the tap is
    the input of the graph's last conv2d call, rpn_conv's), the plain step and the joint step."""
    case = full_case

    @contextlib.contextmanager
    def conv_inputs():
        seen, real = [], TF.conv2d

        def spy(x, *a, **k):
            seen.append(x)
            return real(x, *a, **k)
        TF.conv2d = spy
        try:
            yield seen
        finally:
            TF.conv2d = real

    def graph(dtype, G):
        with conv_inputs() as seen:
            p, r, c, _, _ = mf.full_graph(case["imgs"], case["w"], case["deltas"], case["labels"], True, dtype)
        feat = seen[-1]                                                          # NCHW, the tensor rpn_conv reads
        assert len(seen) == 41 and tuple(feat.shape) == (mf.BATCH, 576, 3, 3)
        if G is None:
            return torch.autograd.grad(r + c, feat)[0].permute(0, 2, 3, 1)
        (r + c + (torch.tensor(G.astype(np.float64)).to(dtype).permute(0, 3, 1, 2) * feat).sum()).backward()
        return p

    g_rpn = graph(torch.float64, None)
    G = seeded_G(tuple(g_rpn.shape), float(g_rpn.abs().mean()))
    batch = (case["imgs"], case["deltas"], case["labels"])
    plain = step(mf.fresh(case), batch, "plain")
    m = mf.fresh(case)
    joint = step(m, batch, "split", torch.from_numpy(G).cuda())
    return dict(G=G, p64=graph(torch.float64, G), p32=graph(torch.float32, G), plain=plain, joint=joint, grads=m.get_gradients(),
                g_rpn_mean=float(g_rpn.abs().mean()))


@pytest.mark.gpu
def test_head_gradients_are_independent_of_the_addend_mobilenet(lib, mn_joint):
    plain, joint = mn_joint["plain"][1], mn_joint["joint"][1]
    for name in HEAD_LAYERS:
        for key in ("kernel", "bias"):
            assert joint[(name, key)] == plain[(name, key)], (name, key)
    assert joint[("block_13_expand", "kernel")] != plain[("block_13_expand", "kernel")]
    assert joint[("block_13_expand_BN", "gamma")] != plain[("block_13_expand_BN", "gamma")]
    assert joint[("Conv1", "kernel")] != plain[("Conv1", "kernel")]


# ---- GPU 4: the chain rule against float64 ------------------------------------------------------------------------------------------
def rel(got, g64):
    return float(np.abs(np.asarray(got, np.float64) - g64).max() / np.abs(g64).max())


@pytest.mark.gpu
def test_joint_gradients_match_float64_autograd_vgg16(lib, vgg_case):
    """Every gradient of r + c + sum(G * feat), G seeded normal x the RPN's mean |gradient| at the tap, against torch float64
    autograd, relative to max |g64| of each tensor; bound per group = 4 x the worst deviation torch float32 CPU autograd of the same
    graph shows in that group (4: the float32 rounding difference of two summation orders, as in test_train_mobilenet_full.py).
    Groups: block5_* and the head (float32 rounding only), and block4_conv3 and below (a max-pool window whose two largest entries
    differ by less than the float32 forward's rounding routes its gradient to another pixel).
    Measured on the MI355X (mean |G| 8.06e-5): block5 + head: torch float32 worst 1.24e-6 (rpn_reg's kernel), bound 4.97e-6, this
    step's worst 1.29e-6 at the same tensor; block4_conv3 and below: torch float32 worst 1.57e-2 (block4_conv3's kernel), bound
    6.29e-2, this step's worst 1.57e-2 at the same tensor."""
    case = vgg_case
    grads = case["joint_grads"]
    top = tuple(n for n in VGG16_CONVS if n.startswith("block5")) + HEAD_LAYERS
    report = {}
    for group, names in (("block5 + head", top), ("block4_conv3 and below", tuple(n for n in VGG16_CONVS if n not in top))):
        t32, ours = {}, {}
        for name in names:
            for i, key in enumerate(("kernel", "bias")):
                g64 = case["p64"][name][i].grad.numpy()
                t32[(name, key)] = rel(case["p32"][name][i].grad.numpy(), g64)
                ours[(name, key)] = rel(grads[name][key], g64)
        bound = 4.0 * max(t32.values())
        worst = max(ours, key=ours.get)
        print("joint VGG16, %s: torch float32 worst %.3g at %s -> bound %.3g; this step's worst %.3g at %s (mean |G| %.3g)"
              % (group, max(t32.values()), max(t32, key=t32.get), bound, ours[worst], worst, case["g_rpn_mean"]))
        report[group] = (ours, bound)
    for group, (ours, bound) in report.items():
        for key, v in ours.items():
            assert v <= bound, (group, key, v, bound)


@pytest.mark.gpu
def test_joint_gradients_match_float64_autograd_mobilenet(lib, full_case, mn_joint):
    """The same on whole MobileNetV2 (one group, test_train_mobilenet_full.py's convention and its grad_devs).
    Measured on the MI355X (mean |G| 9.26e-4): torch float32 worst 8.86e-6 (block_3_depthwise_BN's gamma), bound 3.54e-5, this
    step's worst 7.32e-6 (bn_Conv1's beta)."""
    t32 = mf.grad_devs(mn_joint["p32"], mn_joint["p64"], full_case["flat_beta"])
    devs = mf.grad_devs(mn_joint["grads"], mn_joint["p64"], full_case["flat_beta"])
    assert set(mn_joint["grads"]) == set(mn_joint["p64"])
    bound = 4.0 * max(t32.values())
    worst = max(devs, key=devs.get)
    print("joint MobileNetV2: torch float32 worst %.3g at %s -> bound %.3g; this step's worst %.3g at %s (mean |G| %.3g)"
          % (max(t32.values()), max(t32, key=t32.get), bound, devs[worst], worst, mn_joint["g_rpn_mean"]))
    for key, v in devs.items():
        assert v <= bound, (key, v, bound)


# ---- GPU 5: truncation ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_truncated_joint_backward_gives_the_same_bits(lib, vgg_case):
    case = vgg_case
    part = step(fresh_vgg(case, "block4_conv1"), case["batch"], "split", case["Gd"])
    assert part[0] == case["joint"][0]
    assert set(k[0] for k in part[1]) == set(VGG16_CONVS[7:] + HEAD_LAYERS)
    for key, v in part[1].items():
        assert v == case["joint"][1][key], key


# ---- GPU 6: through the pool, with torch autograd -----------------------------------------------------------------------------------
def pool_inputs():
    rng = np.random.RandomState(8)
    y1, x1 = rng.uniform(0.0, 0.5, (2, 6)), rng.uniform(0.0, 0.5, (2, 6))
    boxes = np.stack([y1, x1, y1 + rng.uniform(0.1, 0.5, (2, 6)), x1 + rng.uniform(0.1, 0.5, (2, 6))], -1).astype(np.float32)
    Wt = rng.standard_normal((2, 6, 3, 3, 512)).astype(np.float32) * np.float32(1e-3)
    return torch.from_numpy(boxes).cuda(), torch.tensor([6, 4], dtype=torch.int32, device="cuda"), torch.from_numpy(Wt).cuda()


@pytest.mark.gpu
def test_second_stage_through_the_pool(lib, vgg_case):
    case = vgg_case
    imgs, deltas, labels = case["batch"]
    boxes, valid, Wt = pool_inputs()
    m = fresh_vgg(case)
    out = m.train_on_batch(imgs, (deltas, labels), second_stage=lambda feat, reg, cls: (roi_pooling(feat, boxes, (3, 3), valid=valid) * Wt).sum())
    auto = (grad_bytes(m), state(m))
    assert len(out) == 4 and m.train_steps() == 1
    assert np.float32(out[0]) == np.float32(out[1]) + np.float32(out[2]) + np.float32(out[3])
    assert np.asarray(out[:3], np.float32)[1:].tobytes() == np.frombuffer(case["plain"][0], np.float32)[1:].tobytes()
    # by hand: the adjoint of the pool applied to d(sum(pool * Wt)) / dpool = Wt
    m = fresh_vgg(case)
    losses, feat, _ = m.forward_for_training(imgs, (deltas, labels))
    want = (roi_pooling(feat, boxes, (3, 3), valid=valid) * Wt).sum().item()
    G = roi_pooling_backward(Wt, boxes, tuple(feat.shape), valid)
    assert G[1].abs().sum().item() > 0 and G.is_contiguous()
    m.apply_gradients(G)
    assert (grad_bytes(m), state(m)) == auto
    assert out[3] == want
    assert auto[0][("block5_conv3", "kernel")] != case["plain"][1][("block5_conv3", "kernel")]
    # a second stage that ignores feat: feat.grad is None, the step is the plain one
    m = fresh_vgg(case)
    free = torch.nn.Parameter(torch.tensor(1.5, device="cuda"))
    out2 = m.train_on_batch(imgs, (deltas, labels), second_stage=lambda feat, reg, cls: free * free)
    assert (grad_bytes(m), state(m)) == case["plain"][1:]
    assert out2[3] == 2.25 and free.grad.item() == 3.0
    assert np.asarray(out2[1:3], np.float32).tobytes() == np.frombuffer(case["plain"][0], np.float32)[1:].tobytes()


# ---- GPU 7: determinism and state -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_joint_step_is_deterministic_and_stateful(lib, vgg_case):
    case = vgg_case
    imgs, deltas, labels = case["batch"]
    m = fresh_vgg(case, learning_rate=1e-4)
    assert m.train_steps() == 0
    m.forward_for_training(imgs, (deltas, labels))
    assert m.train_steps() == 0                                                  # t advances in the backward only
    m.apply_gradients(case["Gd"])
    assert m.train_steps() == 1
    with pytest.raises(RuntimeError, match="pending"):
        m.apply_gradients(case["Gd"])                                            # each forward is applied once
    m.forward_for_training(imgs, (deltas, labels))
    m.test_on_batch(imgs, (deltas, labels))                                      # an evaluation leaves nothing pending
    with pytest.raises(RuntimeError, match="pending"):
        m.apply_gradients()
    # ... and the library says the same to a caller that kept no state of its own
    x = torch.from_numpy(imgs).cuda()
    assert lib.rpn_head_trainer_backward(m._t, L.ptr(x), case["B"], None, *ADAM, L.stream_ptr()) == L.RPN_ERR_INVALID
    assert b"no pending" in lib.rpn_last_error()
    losses, feat, _ = m.forward_for_training(x, (deltas, labels))
    assert lib.rpn_head_trainer_backward(m._t, L.ptr(x), 1, None, *ADAM, L.stream_ptr()) == L.RPN_ERR_INVALID     # another B
    assert b"pending forward ran 2" in lib.rpn_last_error()
    m.apply_gradients(case["Gd"])
    assert m.train_steps() == 2
    first = (grad_bytes(m), state(m))
    # the same two joint steps from the same state: the same bytes
    m = fresh_vgg(case, learning_rate=1e-4)
    for _ in range(2):
        m.forward_for_training(imgs, (deltas, labels))
        m.apply_gradients(case["Gd"])
    assert (grad_bytes(m), state(m)) == first
    # inference after a joint step runs the trained backbone (the bound of test_inference_after_backbone_training)
    _, (reg, cls) = m.test_on_batch(imgs, (deltas, labels), return_outputs=True)
    p_reg, p_cls = m.predict_on_batch(x)
    assert (p_reg - reg).abs().max().item() <= 1e-5 and (p_cls - cls).abs().max().item() <= 1e-5
    m.set_weights(case["w0"])
    q_reg, _ = m.predict_on_batch(x)
    assert not torch.equal(q_reg, p_reg)                                         # (the steps changed what the handle computes)


# ---- GPU 8: it trains -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_joint_training_reduces_the_second_stage_loss(lib, vgg_case):
    case = vgg_case
    imgs, deltas, labels = case["batch"]
    boxes, valid, _ = pool_inputs()
    target = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, (2, 6, 4)).astype(np.float32)).cuda()

    def make_head():
        torch.manual_seed(0)
        head = torch.nn.Linear(3 * 3 * 512, 4).cuda()
        return head, torch.optim.Adam(head.parameters(), lr=1e-3)

    def loss_of(head, feat):
        pooled = roi_pooling(feat, boxes, (3, 3), valid=valid)
        return ((head(pooled.flatten(2)) - target) ** 2).mean()

    def evaluate(m, head):
        m.test_on_batch(imgs, (deltas, labels))
        feat = torch.empty((2, 15, 15, 512), device="cuda")
        L.check(lib.rpn_head_trainer_feature(m._t, L.ptr(feat), 2, L.stream_ptr()), "rpn_head_trainer_feature")   # after train = 0 too
        with torch.no_grad():
            return loss_of(head, feat).item()

    m = fresh_vgg(case, learning_rate=1e-4)
    head, opt = make_head()
    before = evaluate(m, head)
    for _ in range(30):
        opt.zero_grad()
        out = m.train_on_batch(imgs, (deltas, labels), second_stage=lambda feat, reg, cls: loss_of(head, feat))
        opt.step()
    after = evaluate(m, head)
    print("joint training: second-stage loss %.4g -> %.4g, last step %s" % (before, after, out))
    assert np.isfinite(after) and after < before and m.train_steps() == 30
    joint_w = m.get_weights()["block5_conv3"]["kernel"].tobytes()
    # the same loop with the feature gradient withheld: block5_conv3 moves differently
    m = fresh_vgg(case, learning_rate=1e-4)
    head, opt = make_head()
    for _ in range(30):
        opt.zero_grad()
        _, feat, _ = m.forward_for_training(imgs, (deltas, labels))
        loss_of(head, feat).backward()
        m.apply_gradients(None)
        opt.step()
    assert m.get_weights()["block5_conv3"]["kernel"].tobytes() != joint_w


@pytest.mark.gpu
def test_fit_passes_the_second_stage_through(lib, vgg_case):
    case = vgg_case
    imgs, deltas, labels = case["batch"]
    boxes, valid, Wt = pool_inputs()
    second = lambda feat, reg, cls: (roi_pooling(feat, boxes, (3, 3), valid=valid) * Wt).sum()
    m = fresh_vgg(case)
    hist = m.fit(iter([(imgs, (deltas, labels))] * 2), steps_per_epoch=2, second_stage=second)
    assert set(hist) == {"loss", "rpn_reg_loss", "rpn_cls_loss", "second_stage_loss"} and m.train_steps() == 2
    assert np.isfinite(hist["second_stage_loss"][0])
    m = fresh_vgg(case)
    assert set(m.fit(iter([(imgs, (deltas, labels))]), steps_per_epoch=1)) == {"loss", "rpn_reg_loss", "rpn_cls_loss"}
