"""CPU suite for the VGG16 backbone's backward in split float16 (rpn_head_trainer_set_backward_precision, rpn_conv3x3_dgrad_x3,
rpn_conv3x3_wgrad_wide_x3, RPNModel.compile(backward_precision="f16x3")): the ABI checks that need no device, the conv emulation of
the arithmetic contract (include/rpn_hip.h, "Training the backbone's backward in split float16") and the a-priori bounds the GPU tests
(tests/test_gpu_backbone_x3.py) use.

The emulation is the detection head's (tests/test_det_head_x3_train_host, `tr`), fed the implicit GEMMs' operands:
  weight gradient:  a = im2col(x) (P x 9 Cin), dz = dy (P x Cout) into tr.emulate_wgrad / tr.wgrad_bound;
  bias gradient:    a = a column of ones (P x 1) into the same two (the kernel forms db as one more GEMM row of ones; the bound
                    also covers a float32 column sum);
  input gradient:   dz = im2col(dy) (P x 9 Cout: column (3 r + s) Cout + co is dy shifted by (r - 1, s - 1), the "flipped" im2col once
                    the kernel is flipped instead), w = W' (Cin x 9 Cout), W'[ci][(3 r + s) Cout + co] = W[2-r][2-s][ci][co], into
                    tr.emulate_dgrad / tr.dgrad_bound.  t over im2col(dy) is t over dy (the centre tap holds every entry), s over W' is s
                    over the whole HWIO kernel.
The weight-gradient bound's accumulation term counts R = the pixel count plus the depth log2(leaves) of the slab tree: each level
is one more float32 addition per output ((3 (R + depth) + 2) U instead of (3 R + 2) U).

Every case the GPU file uses is built here, once, and the emulation is asserted to lie inside the bound on the CPU.
"""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_host as dh  # noqa: E402
import test_det_head_x3_host as hx  # noqa: E402
import test_det_head_x3_train_host as tr  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from test_gpu_backward import dy_like, he_like, relu_like  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402

ROOT = dh.ROOT
U = dh.U
F32, BF16X3, F16X3, F32W = 0, 1, 2, 3
NEW_SYMBOLS = ["rpn_head_trainer_set_backward_precision", "rpn_head_trainer_backward_precision", "rpn_head_trainer_status",
               "rpn_conv3x3_dgrad_x3_workspace_bytes", "rpn_conv3x3_dgrad_x3", "rpn_conv3x3_wgrad_wide_x3_workspace_bytes",
               "rpn_conv3x3_wgrad_wide_x3", "rpn_conv3x3_dgrad_x3_tile_n", "rpn_head_trainer_backward_x3_bytes"]

GRAD_SCALES = (1.0, 2.0 ** -20, 1e-7)
# (B, H, W, Cin, Cout)
DGRAD = [(1, 1, 1, 4, 16), (1, 3, 5, 4, 16), (2, 7, 13, 20, 48), (1, 9, 33, 68, 16), (3, 31, 17, 132, 80), (1, 40, 23, 192, 48),
         (2, 128, 128, 128, 16)]          # the last one: the 128-wide tile (256 pixel tiles x 1)
WGRAD = [(1, 1, 1, 4, 4), (1, 3, 5, 4, 20), (1, 15, 15, 512, 512), (1, 40, 27, 12, 132), (2, 62, 31, 256, 132), (2, 62, 47, 128, 68)]


def a256(n):
    return (n + 255) & ~255


def x3_leaves(lib, B, H, W, Cin, Cout):
    """the leaves rpn_conv3x3_wgrad_wide_x3 splits a shape into, from its workspace size: a256(L * slab) + 256 bytes of words"""
    total = lib.rpn_conv3x3_wgrad_wide_x3_workspace_bytes(B, H, W, Cin, Cout)
    slab = (9 * Cin + 1) * Cout * 4
    found = [n for n in (1 << k for k in range(11)) if a256(n * slab) + 256 == total]
    assert len(found) == 1, (B, H, W, Cin, Cout, total)
    return found[0]


# ---- the implicit GEMMs' operands ----------------------------------------------------------------------------------------------------------
def im2col(x):
    """(B,H,W,C) -> (B H W, 9 C): column (3 r + s) C + c of pixel (b, y, x) is x[b][y + r - 1][x + s - 1][c], zero outside"""
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    return np.concatenate([xp[:, r:r + H, s:s + W].reshape(B * H * W, C) for r in range(3) for s in range(3)], axis=1)


def flipped_kernel(w):
    """HWIO (3,3,Cin,Cout) -> W' (Cin, 9 Cout): W'[ci][(3 r + s) Cout + co] = w[2 - r][2 - s][ci][co]"""
    return np.concatenate([w[2 - r, 2 - s] for r in range(3) for s in range(3)], axis=1)


def emulate_conv_wgrad(x, dy, parts=(1, 1, 1), t=None):
    """the contract's (dw (3,3,Cin,Cout), db (Cout)) in float64"""
    Cin, Cout = x.shape[3], dy.shape[3]
    dz = dy.reshape(-1, Cout)
    dw = tr.emulate_wgrad(im2col(x), dz, parts=parts, t=t).reshape(3, 3, Cin, Cout)
    return dw, tr.emulate_wgrad(np.ones((dz.shape[0], 1), np.float32), dz, parts=parts, t=t)[0]


def conv_wgrad_bound(x, dy, leaves=1, edy=None, final=True):
    """(bound of dw, bound of db) for float64 x, dy; edy: the error dy's float32 counterpart already carries"""
    Cin, Cout = x.shape[3], dy.shape[3]
    a, dz = np.abs(im2col(np.asarray(x, np.float64))), np.abs(np.asarray(dy, np.float64).reshape(-1, Cout))
    edz = None if edy is None else np.asarray(edy, np.float64).reshape(-1, Cout)
    depth = int(math.log2(leaves))
    ones = np.ones((dz.shape[0], 1))
    ew = tr.wgrad_bound(a, dz, edz=edz, final=False) + 3 * depth * U * (a.T @ dz)
    eb = tr.wgrad_bound(ones, dz, edz=edz, final=False) + 3 * depth * U * (ones.T @ dz)
    k = 2.0 if final else 1.0
    return k * ew.reshape(3, 3, Cin, Cout), k * eb[0]


def emulate_conv_dgrad(dy, w, mask=None, add=None, parts=(1, 1, 1), t=None):
    """the contract's dx (B,H,W,Cin) in float64: mask > 0 ? product + add : 0"""
    B, H, W, _ = dy.shape
    out = tr.emulate_dgrad(im2col(dy), flipped_kernel(w), parts=parts, t=t).reshape(B, H, W, w.shape[2])
    if add is not None:
        out = out + np.asarray(add, np.float64)
    return out if mask is None else out * (np.asarray(mask) > 0)


def conv_dgrad_bound(dy, w, edy=None, add=None, final=True):
    """bound of dx for float64 dy, w; with `add` the one more float32 rounding of fl32(product + add)"""
    B, H, W, _ = dy.shape
    dy64, w64 = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    edz = None if edy is None else im2col(np.asarray(edy, np.float64))
    a, wf = im2col(dy64), flipped_kernel(w64)
    e = tr.dgrad_bound(a, wf, edz=edz, final=False).reshape(B, H, W, w.shape[2])
    if add is not None:
        e = e + U * (np.abs(a) @ np.abs(wf).T).reshape(e.shape) + U * np.abs(np.asarray(add, np.float64))
    return 2.0 * e if final else e


# ---- cases (built once, read-only) ---------------------------------------------------------------------------------------------------------
_CACHE = {}


def dgrad_case(shape):
    """dy, w, mask, add as the trainer feeds them (tests/test_gpu_backward's builders).  Every image holds one entry equal to the
    tensor's maximum (at [b, 0, 0, 0]), so that an image alone and the batch share t."""
    if ("d", shape) not in _CACHE:
        B, H, W, Cin, Cout = shape
        rng = np.random.RandomState(5000 + B * H + W + Cin + Cout)
        dy, w = dy_like(rng, (B, H, W, Cout)), he_like(rng, Cin, Cout)
        mask, add = relu_like(rng, (B, H, W, Cin)), dy_like(rng, (B, H, W, Cin))
        dy[:, 0, 0, 0] = max(np.abs(dy).max(), np.float32(0.25))
        assert all(tr.grad_shift_of(dy[b]) == tr.grad_shift_of(dy) for b in range(B))
        _CACHE[("d", shape)] = hx._frozen(dict(dy=dy, w=w, mask=mask, add=add))
    return _CACHE[("d", shape)]


def wgrad_case(shape):
    if ("w", shape) not in _CACHE:
        B, H, W, Cin, Cout = shape
        rng = np.random.RandomState(6000 + B + H + W + Cin + Cout)
        x, dy = relu_like(rng, (B, H, W, Cin)), dy_like(rng, (B, H, W, Cout))
        dy[0, 0, 0, 0] = max(np.abs(dy).max(), np.float32(0.25))           # (one pixel can draw an all-zero dy)
        x[0, 0, 0, 0] = max(x[0, 0, 0, 0], np.float32(0.5))
        _CACHE[("w", shape)] = hx._frozen(dict(x=x, dy=dy))
    return _CACHE[("w", shape)]


def dgrad_reference(c, scale, use_mask, use_add):
    """(dy, add, float64 reference, bound) of one dgrad case at a gradient scale; the addend is scaled with the gradient.  The
    product's reference and bound are computed once per (case, scale) and shared by the mask / add variants."""
    from test_train_backbone import dgrad64
    key = ("dref", id(c["dy"]), scale)
    if key not in _CACHE:
        dy = tr.scaled(c["dy"], scale)
        dy64, w64 = dy.astype(np.float64), c["w"].astype(np.float64)
        _CACHE[key] = (dy, dgrad64(dy64, w64), conv_dgrad_bound(dy, c["w"], final=False), dgrad64(np.abs(dy64), np.abs(w64)))
    dy, ref, e, absprod = _CACHE[key]
    add = tr.scaled(c["add"], scale) if use_add else None
    if use_add:                               # fl32(product + add): one more rounding (conv_dgrad_bound's add term)
        ref, e = ref + add.astype(np.float64), e + U * absprod + U * np.abs(add.astype(np.float64))
    bound = 2.0 * e
    if use_mask:
        keep = c["mask"] > 0
        ref, bound = ref * keep, bound * keep
    return dy, add, ref, bound


def exact_dgrad_case(shape):
    """small integers in w, dy = small integers times 2^-5: every lo half is 0 and every float32 partial sum exact (|sum| <= 4 * 9 *
    Cout integers times one power of two, far below 2^24)"""
    B, H, W, Cin, Cout = shape
    rng = np.random.RandomState(7000 + H + W + Cin)
    dy = (rng.randint(-2, 3, size=(B, H, W, Cout)) * 2.0 ** -5).astype(np.float32)
    dy[:, 0, 0, 0] = 2.0 ** -4
    w = rng.randint(-2, 3, size=(3, 3, Cin, Cout)).astype(np.float32)
    w[0, 0, 0, 0] = 2.0
    mask = rng.choice(np.array([-1.5, -0.0, 0.0, 0.5, 2.0], np.float32), size=(B, H, W, Cin))
    add = (rng.randint(-3, 4, size=(B, H, W, Cin)) * 2.0 ** -5).astype(np.float32)
    return dict(dy=dy, w=w, mask=mask, add=add)


def exact_wgrad_case(shape):
    """small integers in x, dy = small integers times 2^-5: |sums| <= 4 B H W integers times one power of two, below 2^24"""
    B, H, W, Cin, Cout = shape
    rng = np.random.RandomState(8000 + H + W + Cin)
    x = rng.randint(-2, 3, size=(B, H, W, Cin)).astype(np.float32)
    dy = (rng.randint(-2, 3, size=(B, H, W, Cout)) * 2.0 ** -5).astype(np.float32)
    dy[0, 0, 0, 0] = 2.0 ** -4
    return dict(x=x, dy=dy)


def _ratio(z, ref, bound):
    return float((np.abs(z - ref) / np.maximum(bound, 1e-300)).max())


# ---- 1. the emulation and the bounds -----------------------------------------------------------------------------------------------------
def test_operands_restate_the_float64_references():
    from test_train_backbone import dgrad64, wgrad64
    rng = np.random.RandomState(3)
    x, dy, w = relu_like(rng, (2, 5, 4, 8)), dy_like(rng, (2, 5, 4, 16)), he_like(rng, 8, 16)
    x64, dy64, w64 = x.astype(np.float64), dy.astype(np.float64), w.astype(np.float64)
    dw, db = wgrad64(x64, dy64)
    assert np.allclose(im2col(x64).T @ dy64.reshape(-1, 16), dw.reshape(72, 16), rtol=1e-13, atol=0)
    assert np.allclose(dy64.reshape(-1, 16).sum(0), db, rtol=1e-13, atol=0)
    assert np.allclose((im2col(dy64) @ flipped_kernel(w64).T).reshape(2, 5, 4, 8), dgrad64(dy64, w64), rtol=1e-12, atol=1e-300)
    assert tr.grad_shift_of(im2col(dy)) == tr.grad_shift_of(dy) and hx.shift_of(flipped_kernel(w)) == hx.shift_of(w)


@pytest.mark.parametrize("shape", DGRAD)
def test_dgrad_emulation_lies_inside_the_bound(shape):
    c = dgrad_case(shape)
    worst = 0.0
    for scale in GRAD_SCALES:
        for use_mask, use_add in ((False, False), (True, True)):
            dy, add, ref, bound = dgrad_reference(c, scale, use_mask, use_add)
            emu = emulate_conv_dgrad(dy, c["w"], c["mask"] if use_mask else None, add)
            r = _ratio(emu, ref, bound)
            assert r <= 1.0, (shape, scale, use_mask, r)
            worst = max(worst, r)
    print("dgrad %s: worst emulation error / bound %.3f" % (shape, worst))
    assert 0.0 < worst


@pytest.mark.parametrize("shape", WGRAD)
def test_wgrad_emulation_lies_inside_the_bound(lib, shape):
    from test_train_backbone import wgrad64
    c = wgrad_case(shape)
    leaves = x3_leaves(lib, *shape)
    worst = 0.0
    for scale in GRAD_SCALES:
        dy = tr.scaled(c["dy"], scale)
        ref_w, ref_b = wgrad64(c["x"].astype(np.float64), dy.astype(np.float64))
        bw, bb = conv_wgrad_bound(c["x"], dy, leaves)
        dw, db = emulate_conv_wgrad(c["x"], dy)
        r = max(_ratio(dw, ref_w, bw), _ratio(db, ref_b, bb))
        assert r <= 1.0, (shape, scale, r)
        worst = max(worst, r)
    print("wgrad %s (%d leaves): worst emulation error / bound %.3f" % (shape, leaves, worst))
    assert 0.0 < worst


def test_shape_tables_reach_every_path(lib):
    leaves = {s: x3_leaves(lib, *s) for s in WGRAD}
    assert 1 in leaves.values() and 2 in leaves.values() and any(v >= 4 for v in leaves.values()), leaves
    tiles = {s: lib.rpn_conv3x3_dgrad_x3_tile_n(*s[:4]) for s in DGRAD}
    assert set(tiles.values()) == {64, 128}, tiles
    assert {s[4] for s in DGRAD} >= {16, 48, 80}                  # a step of 32 meets a tap boundary
    assert any(s[3] % 64 for s in DGRAD) and any(s[0] * s[1] * s[2] % 128 for s in DGRAD) and any(s[0] * s[1] * s[2] == 1 for s in DGRAD)
    assert any((9 * s[3] + 1) % 128 == 1 for s in WGRAD) and any(s[4] % 128 for s in WGRAD) and any(s[4] % 128 == 0 for s in WGRAD)


def test_the_bounds_notice_a_dropped_product():
    from test_train_backbone import dgrad64, wgrad64
    c = wgrad_case((1, 3, 5, 4, 20))          # (15 pixels: over a long reduction the accumulation term outgrows a dropped product)
    ref_w, _ = wgrad64(c["x"].astype(np.float64), c["dy"].astype(np.float64))
    bw, _ = conv_wgrad_bound(c["x"], c["dy"], 1)
    for parts in ((1, 0, 1), (1, 1, 0), (0, 1, 1)):
        assert (np.abs(emulate_conv_wgrad(c["x"], c["dy"], parts=parts)[0] - ref_w) > bw).any(), parts
    c = dgrad_case((2, 7, 13, 20, 48))
    ref = dgrad64(c["dy"].astype(np.float64), c["w"].astype(np.float64))
    bound = conv_dgrad_bound(c["dy"], c["w"])
    for parts in ((1, 0, 1), (1, 1, 0), (0, 1, 1)):
        assert (np.abs(emulate_conv_dgrad(c["dy"], c["w"], parts=parts) - ref) > bound).any(), parts


def test_the_bounds_notice_a_missing_gradient_shift():
    """at gradient scale 1e-7 the unshifted split (t = 0) loses the lo halves to float16's subnormals and leaves the bound"""
    from test_train_backbone import dgrad64, wgrad64
    c = wgrad_case((1, 3, 5, 4, 20))
    dy = tr.scaled(c["dy"], 1e-7)
    assert tr.grad_shift_of(dy) >= 33
    ref_w, ref_b = wgrad64(c["x"].astype(np.float64), dy.astype(np.float64))
    bw, bb = conv_wgrad_bound(c["x"], dy, 1)
    dw, db = emulate_conv_wgrad(c["x"], dy, t=0)
    assert (np.abs(dw - ref_w) > bw).any() and (np.abs(db - ref_b) > bb).any()
    c = dgrad_case((2, 7, 13, 20, 48))
    dy = tr.scaled(c["dy"], 1e-7)
    ref = dgrad64(dy.astype(np.float64), c["w"].astype(np.float64))
    assert (np.abs(emulate_conv_dgrad(dy, c["w"], t=0) - ref) > conv_dgrad_bound(dy, c["w"])).any()


def test_exact_cases_are_exact_under_the_contract():
    from test_train_backbone import dgrad64, wgrad64
    c = exact_dgrad_case((2, 7, 13, 20, 48))
    assert tr.grad_shift_of(c["dy"]) == 15 and hx.shift_of(c["w"]) == 10
    ref = dgrad64(c["dy"].astype(np.float64), c["w"].astype(np.float64))
    assert np.array_equal(emulate_conv_dgrad(c["dy"], c["w"]), ref) and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    assert not np.array_equal(emulate_conv_dgrad(c["dy"], c["w"], parts=(0, 1, 1)), ref)
    c = exact_wgrad_case((1, 40, 27, 12, 132))
    ref_w, ref_b = wgrad64(c["x"].astype(np.float64), c["dy"].astype(np.float64))
    dw, db = emulate_conv_wgrad(c["x"], c["dy"])
    assert np.array_equal(dw, ref_w) and np.array_equal(db, ref_b)


# ---- 2. ABI without a device -------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    assert "Training the backbone's backward in split float16" in header
    assert lib.rpn_abi_version() == 1


def _model(backbone="vgg16", img=96, F=6):
    from oracle import bbox_oracle as bo
    from tf_rpn_amd.models._rpn_model import RPNModel
    hp = bo.get_hyper_params(backbone, img_size=img, feature_map_shape=F)
    return RPNModel(backbone, hp, max_batch=2)


def test_set_backward_precision_argument_and_state_checks_need_no_device(lib):
    m = _model()
    t = L.vp(0)
    assert lib.rpn_model_trainer_create(m._h, b"block3_conv1", ctypes.byref(t)) == L.RPN_OK
    try:
        assert lib.rpn_head_trainer_backward_precision(t) == F32
        for bad in (-1, 4, 17):
            assert lib.rpn_head_trainer_set_backward_precision(t, bad) == L.RPN_ERR_INVALID
        assert b"rpn_head_trainer_set_backward_precision" in lib.rpn_last_error()
        for unsupported in (BF16X3, F32W):
            assert lib.rpn_head_trainer_set_backward_precision(t, unsupported) == L.RPN_ERR_UNSUPPORTED
        assert lib.rpn_head_trainer_backward_precision(t) == F32
        assert lib.rpn_head_trainer_set_backward_precision(t, F16X3) == L.RPN_OK and lib.rpn_head_trainer_backward_precision(t) == F16X3
        assert lib.rpn_head_trainer_steps(t) == 0
        flags = ctypes.c_uint(7)
        assert lib.rpn_head_trainer_status(t, ctypes.byref(flags), 1, None) == L.RPN_OK and flags.value == 0
        assert lib.rpn_head_trainer_status(t, None, 0, None) == L.RPN_ERR_INVALID
        assert lib.rpn_head_trainer_set_backward_precision(t, F32) == L.RPN_OK and lib.rpn_head_trainer_backward_precision(t) == F32
        # the image of the largest trained layer (block 4 / 5 / rpn_conv: 9 * 512 / 32 chunks of 512 records of 128 bytes) + 64 words
        assert lib.rpn_head_trainer_backward_x3_bytes(t) == 144 * 512 * 128 + 256
    finally:
        lib.rpn_head_trainer_destroy(t)
    assert lib.rpn_head_trainer_set_backward_precision(None, F32) == L.RPN_ERR_INVALID
    assert lib.rpn_head_trainer_backward_precision(None) == F32 and lib.rpn_head_trainer_backward_x3_bytes(None) == 0
    # a head-only trainer and a MobileNetV2 trainer: F32 only
    t = L.vp(0)
    assert lib.rpn_head_trainer_create(m._h, ctypes.byref(t)) == L.RPN_OK
    try:
        assert lib.rpn_head_trainer_set_backward_precision(t, F16X3) == L.RPN_ERR_UNSUPPORTED and b"head only" in lib.rpn_last_error()
        assert lib.rpn_head_trainer_set_backward_precision(t, F32) == L.RPN_OK and lib.rpn_head_trainer_backward_x3_bytes(t) == 0
    finally:
        lib.rpn_head_trainer_destroy(t)
    mn = _model("mobilenet_v2", 96, 6)
    t = L.vp(0)
    assert lib.rpn_model_trainer_create(mn._h, b"block_13_expand", ctypes.byref(t)) == L.RPN_OK
    try:
        assert lib.rpn_head_trainer_set_backward_precision(t, F16X3) == L.RPN_ERR_UNSUPPORTED and b"MobileNetV2" in lib.rpn_last_error()
        assert lib.rpn_head_trainer_backward_precision(t) == F32
    finally:
        lib.rpn_head_trainer_destroy(t)


def test_entries_validate_before_device_use(lib):
    keep, p = dh._aligned()
    odd, half = L.vp(p.value + 4), L.vp(p.value + 2)
    big = 1 << 30

    def dg(dy=p, w=p, mask=None, add=None, B=1, H=2, W=2, Cin=4, Cout=16, dx=p, status=None, ws=p, n=big):
        return lib.rpn_conv3x3_dgrad_x3(dy, w, mask, add, B, H, W, Cin, Cout, dx, status, ws, n, None)

    for bad in (dict(dy=None), dict(w=None), dict(dx=None), dict(B=0), dict(H=0), dict(W=0), dict(Cin=0), dict(Cin=6), dict(Cout=8),
                dict(Cout=24), dict(dy=odd), dict(w=half), dict(ws=odd), dict(dx=half), dict(mask=half), dict(add=half), dict(status=half),
                dict(Cin=1 << 16, Cout=1 << 16)):
        assert dg(**bad) == L.RPN_ERR_INVALID, bad
    assert b"rpn_conv3x3_dgrad_x3" in lib.rpn_last_error()
    assert dg(ws=None) == L.RPN_ERR_WORKSPACE and dg(n=lib.rpn_conv3x3_dgrad_x3_workspace_bytes(4, 16) - 1) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_conv3x3_dgrad_x3_workspace_bytes(4, 16) == a256(5 * 4 * 128) + 256       # 144 / 32 -> 5 chunks
    assert lib.rpn_conv3x3_dgrad_x3_workspace_bytes(6, 16) == 0 and lib.rpn_conv3x3_dgrad_x3_workspace_bytes(4, 8) == 0
    assert lib.rpn_conv3x3_dgrad_x3_tile_n(0, 1, 1, 4) == 0
    # a kernel needs 4-byte alignment only (the trainer's master kernels are slices of one flat buffer): such a call passes the
    # validation (these are host pointers: asked only where no device could be handed them;
    # tests/test_gpu_backbone_x3.py runs an unaligned kernel on the device)
    import torch
    if not torch.cuda.is_available():
        assert dg(w=odd) == L.RPN_ERR_NO_DEVICE

    def wg(x=p, dy=p, B=1, H=2, W=2, Cin=4, Cout=4, dw=p, db=p, status=None, ws=p, n=big):
        return lib.rpn_conv3x3_wgrad_wide_x3(x, dy, B, H, W, Cin, Cout, dw, db, status, ws, n, None)

    for bad in (dict(x=None), dict(dy=None), dict(dw=None), dict(db=None), dict(B=0), dict(H=0), dict(Cin=6), dict(Cin=0), dict(Cout=6),
                dict(Cout=0), dict(x=odd), dict(dy=odd), dict(ws=odd), dict(dw=half), dict(db=half), dict(status=half),
                dict(B=1 << 10, H=1 << 11, W=1 << 10)):
        assert wg(**bad) == L.RPN_ERR_INVALID, bad
    assert b"rpn_conv3x3_wgrad_wide_x3" in lib.rpn_last_error()
    assert wg(Cin=3) == L.RPN_ERR_UNSUPPORTED and b"block1_conv1" in lib.rpn_last_error()
    assert wg(ws=None) == L.RPN_ERR_WORKSPACE and wg(n=16) == L.RPN_ERR_WORKSPACE
    assert lib.rpn_conv3x3_wgrad_wide_x3_workspace_bytes(1, 2, 2, 3, 4) == 0
    assert lib.rpn_conv3x3_wgrad_wide_x3_workspace_bytes(1, 2, 2, 4, 4) == a256(37 * 4 * 4) + 256
    if not torch.cuda.is_available():
        assert dg() == L.RPN_ERR_NO_DEVICE and wg() == L.RPN_ERR_NO_DEVICE
    del keep


def test_python_compile_backward_precision_checks():
    m = _model()
    assert m.backward_precision == "f32"
    for bad in ("bf16x3", "f32w", "fp16", None, 2):
        with pytest.raises(ValueError, match="backward_precision"):
            m.compile(train_backbone_from="block4_conv1", backward_precision=bad)
    with pytest.raises(ValueError, match="head only"):
        m.compile(backward_precision="f16x3")
    with pytest.raises(ValueError, match="mobilenet_v2"):
        _model("mobilenet_v2").compile(train_backbone_from="block_13_expand", backward_precision="f16x3")
    with pytest.raises(ValueError, match="mobilenet_v2"):
        _model("mobilenet_v2").compile(train_backbone=True, backward_precision="f16x3")
    with pytest.raises(RuntimeError):
        m.train_status()


def test_python_compile_f16x3_reports_the_setting(lib):
    from oracle import bbox_oracle as bo
    from tf_rpn_amd.models._rpn_model import RPNModel, synthetic_weights, HEAD_LAYERS, VGG16_CONVS
    hp = bo.get_hyper_params("vgg16", img_size=96, feature_map_shape=6)
    m = RPNModel("vgg16", hp, max_batch=2)
    w = synthetic_weights("vgg16", hp, seed=3)
    for name in HEAD_LAYERS:
        m._head[name] = (w[name]["kernel"], w[name]["bias"])
    for name in VGG16_CONVS:
        m._backbone[name] = (w[name]["kernel"], w[name]["bias"])
    m.compile(train_backbone_from="block4_conv1", backward_precision="f16x3")
    assert m.backward_precision == "f16x3" and m.train_status() == {"f16_range": False}
    assert m.trained_layers() == tuple(VGG16_CONVS[7:]) + tuple(HEAD_LAYERS)
    m.compile(train_backbone=True, backward_precision="f16x3")
    assert m.backward_precision == "f16x3" and m.train_steps() == 0
    m.compile(train_backbone=True)
    assert m.backward_precision == "f32"


def test_backbone_x3_kernel_budgets(lib):
    """the two GEMMs keep their accumulators, fragments and staging without scratch, in at most 64 KB of LDS (two workgroups per CU)
    and 256 threads; the register counts are pinned at what the build gives: 188 (wgrad), 188 (dgrad, 128-wide), 132 (dgrad, 64-wide)
    -- two workgroups of four waves per CU need at most 256"""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    pins = {"conv3x3_wgrad_x3_kernel": 188, "conv3x3_dgrad_x3_kernel<4>": 188, "conv3x3_dgrad_x3_kernel<2>": 132}
    for name, cap in pins.items():
        vgpr, sspill, vspill, scratch, lds, wg = tab[name]
        assert vgpr <= cap and sspill == 0 and vspill == 0 and scratch == 0 and lds <= 64 * 1024 and wg == 256, (name, tab[name])
    for name in ("conv_absmax_x3_kernel", "conv_absmax1_x3_kernel", "dgrad_pack_x3_kernel<true>", "dgrad_pack_x3_kernel<false>"):
        assert tab[name][3] == 0 and tab[name][4] == 0 and tab[name][0] <= 64, (name, tab[name])
    for name in ("fc_forward_x3_kernel", "fc_wgrad_x3_kernel", "fc_dgrad_x3_kernel"):        # the head's kernels after the helpers moved
        vgpr, sspill, vspill, scratch, lds, wg = tab[name]
        assert vgpr <= 184 and sspill == 0 and vspill == 0 and scratch == 0 and lds == 64 * 1024 and wg == 256, (name, tab[name])
