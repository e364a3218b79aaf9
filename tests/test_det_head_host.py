"""CPU suite for the detection head (rpn_det_head_*, rpn_fc_forward, models.DetectionHead): the float64 restatements the GPU tests
compare against, the a-priori float32 error bound they use, and the ABI checks that need no device.

The bound (`bounds`, `product_bound`) is a first-order forward error analysis of float32 arithmetic, u = 2^-24; nothing in it comes
from what the kernels give:
  * a product out = A W + bias of inner length K, summed in ANY order, is off by at most (K + 2) u (|A| |W| + |bias|) elementwise
    (K - 1 additions, one rounding per product -- none under an fma --, the bias addition);
  * an input that already carries the error e contributes e |W| (and, where the other factor carries one too, |A| e_W);
  * ReLU is 1-Lipschitz: it passes an error on unchanged;
  * the backward products dW = A^T dZ and dA = dZ W^T follow the same rule with both factors' errors, |A|^T e_dZ + e_A^T |dZ|;
    a bias gradient is the product with a row of ones;
  * the total is multiplied by 2, for the second-order terms and for rounding the stored intermediates.
The backward bound holds where the float32 and the float64 ReLU masks agree, so every case asserts, on the CPU and from the float64
restatement alone, that no pre-activation lies within its own forward bound of zero; the seeds are chosen so that this holds.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as entry  # noqa: E402
import test_roi_head_host as rh  # noqa: E402
import test_roi_host as rp  # noqa: E402
from test_train import adam64  # noqa: E402,F401  (the GPU tests take it from here)
from tf_rpn_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
LAYERS = ("fc1", "fc2", "cls", "reg")
NEW_SYMBOLS = ["rpn_det_head_adam_step", "rpn_det_head_backward", "rpn_det_head_create", "rpn_det_head_destroy", "rpn_det_head_forward",
               "rpn_det_head_get_gradient", "rpn_det_head_get_layer", "rpn_det_head_memory_bytes", "rpn_det_head_set_layer",
               "rpn_det_head_steps", "rpn_fc_forward"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


# ---- restatements -------------------------------------------------------------------------------------------------------------------
def _w64(weights):
    return {n: {k: np.asarray(v, np.float64) for k, v in weights[n].items()} for n in LAYERS}


def det_head_ref(weights, pooled):
    """float64 forward: pooled (B,R,ph,pw,Cf) -> dict(x, z1, h1, z2, h2, logits (B,R,C), deltas (B,R,4C)); x is Keras' Flatten of NHWC"""
    w = _w64(weights)
    p = np.asarray(pooled, np.float64)
    B, R = p.shape[:2]
    x = p.reshape(B * R, -1)                                   # index (i * pw + j) * Cf + c
    z1 = x @ w["fc1"]["kernel"] + w["fc1"]["bias"]
    h1 = np.maximum(z1, 0.0)
    z2 = h1 @ w["fc2"]["kernel"] + w["fc2"]["bias"]
    h2 = np.maximum(z2, 0.0)
    logits = h2 @ w["cls"]["kernel"] + w["cls"]["bias"]
    deltas = h2 @ w["reg"]["kernel"] + w["reg"]["bias"]
    return dict(x=x, z1=z1, h1=h1, z2=z2, h2=h2, logits=logits.reshape(B, R, -1), deltas=deltas.reshape(B, R, -1))


def det_head_backward_ref(weights, pooled, grad_logits, grad_deltas):
    """float64 backward -> ({layer: {"kernel", "bias"}}, grad_pooled (B,R,ph,pw,Cf))"""
    w = _w64(weights)
    f = det_head_ref(weights, pooled)
    M = f["x"].shape[0]
    gl, gd = np.asarray(grad_logits, np.float64).reshape(M, -1), np.asarray(grad_deltas, np.float64).reshape(M, -1)
    g = {"cls": {"kernel": f["h2"].T @ gl, "bias": gl.sum(axis=0)}, "reg": {"kernel": f["h2"].T @ gd, "bias": gd.sum(axis=0)}}
    d2 = (gl @ w["cls"]["kernel"].T + gd @ w["reg"]["kernel"].T) * (f["z2"] > 0)
    g["fc2"] = {"kernel": f["h1"].T @ d2, "bias": d2.sum(axis=0)}
    d1 = (d2 @ w["fc2"]["kernel"].T) * (f["z1"] > 0)
    g["fc1"] = {"kernel": f["x"].T @ d1, "bias": d1.sum(axis=0)}
    return g, (d1 @ w["fc1"]["kernel"].T).reshape(np.shape(pooled))


# ---- the a-priori bound ---------------------------------------------------------------------------------------------------------------
def product_bound(A, W, bias=None, eA=None, eW=None, final=True):
    """Elementwise bound on |fl32(A W + bias) - (A W + bias)| for float64 A (M,K), W (K,N) whose float32 counterparts carry the errors
    eA / eW (None: exact).  `final`: times 2 (module docstring); inner calls of a chain pass False and double once at the end."""
    A, W = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(W, np.float64))
    K = A.shape[1]
    e = (K + 2) * U * (A @ W + (0.0 if bias is None else np.abs(np.asarray(bias, np.float64))))
    if eA is not None:
        e = e + np.asarray(eA, np.float64) @ W
    if eW is not None:
        e = e + A @ np.asarray(eW, np.float64)
    return 2.0 * e if final else e


def bounds(weights, pooled, grad_logits=None, grad_deltas=None, e_grad_logits=None, e_grad_deltas=None):
    """The bound on every output of the head for exactly representable weights and pooled features: "z1", "z2" (pre-activations),
    "logits", "deltas"; with the output gradients given (exact, or carrying e_grad_*) also {layer: {"kernel", "bias"}} and
    "grad_pooled".  Every entry is the doubled total."""
    w = _w64(weights)
    f = det_head_ref(weights, pooled)
    B, R = np.shape(pooled)[:2]
    e1 = product_bound(f["x"], w["fc1"]["kernel"], w["fc1"]["bias"], final=False)          # of z1, and of h1 (ReLU)
    e2 = product_bound(f["h1"], w["fc2"]["kernel"], w["fc2"]["bias"], eA=e1, final=False)
    el = product_bound(f["h2"], w["cls"]["kernel"], w["cls"]["bias"], eA=e2, final=False)
    ed = product_bound(f["h2"], w["reg"]["kernel"], w["reg"]["bias"], eA=e2, final=False)
    out = {"z1": 2 * e1, "z2": 2 * e2, "logits": 2 * el.reshape(B, R, -1), "deltas": 2 * ed.reshape(B, R, -1)}
    if grad_logits is None:
        return out
    M = f["x"].shape[0]
    gl, gd = np.asarray(grad_logits, np.float64).reshape(M, -1), np.asarray(grad_deltas, np.float64).reshape(M, -1)
    egl = np.zeros_like(gl) if e_grad_logits is None else np.asarray(e_grad_logits, np.float64).reshape(M, -1)
    egd = np.zeros_like(gd) if e_grad_deltas is None else np.asarray(e_grad_deltas, np.float64).reshape(M, -1)
    ones = np.ones((1, M))

    def wgrad(a, ea, dz, edz):          # dW = a^T dz and db = 1^T dz, inner length M
        return {"kernel": 2 * product_bound(a.T, dz, eA=None if ea is None else ea.T, eW=edz, final=False),
                "bias": 2 * product_bound(ones, dz, eW=edz, final=False)[0]}

    out["cls"], out["reg"] = wgrad(f["h2"], e2, gl, egl), wgrad(f["h2"], e2, gd, egd)
    # d2 = (gl Wc^T + gd Wr^T) [z2 > 0]: one product of inner length 5 C over the concatenated pair
    dz, edz = np.concatenate([gl, gd], axis=1), np.concatenate([egl, egd], axis=1)
    wp = np.concatenate([w["cls"]["kernel"], w["reg"]["kernel"]], axis=1)
    m2, m1 = f["z2"] > 0, f["z1"] > 0
    d2 = (dz @ wp.T) * m2
    ed2 = product_bound(dz, wp.T, eA=edz, final=False) * m2
    out["fc2"] = wgrad(f["h1"], e1, d2, ed2)
    d1 = (d2 @ w["fc2"]["kernel"].T) * m1
    ed1 = product_bound(d2, w["fc2"]["kernel"].T, eA=ed2, final=False) * m1
    out["fc1"] = wgrad(f["x"], None, d1, ed1)
    out["grad_pooled"] = 2 * product_bound(d1, w["fc1"]["kernel"].T, eA=ed1, final=False).reshape(np.shape(pooled))
    return out


def assert_masks_are_safe(weights, pooled):
    """the condition on the INPUTS under which the backward bound holds (module docstring); the float64 restatement alone decides"""
    f, b = det_head_ref(weights, pooled), bounds(weights, pooled)
    for z in ("z1", "z2"):
        near = np.abs(f[z]) <= b[z]
        assert not near.any(), "%s: %d pre-activations within their forward bound of zero -- choose another seed" % (z, int(near.sum()))


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
# (ph, pw, Cf, H1, H2, C): every tail of the 128 x 128 x 32 forward tile and of the 64-wide backward tiles at the smallest sizes --
# K1 = 108 (a K tail), 68 and 132 wide layers (a tile tail, two tiles and a tail), 5 C = 15 (narrower than a tile, not a multiple of
# 4) and 5 C = 105 (the operating point's width); B x R = 2 x 37 = 74 rows (a row tail)
HEAD_CONFIGS = [(3, 3, 12, 68, 132, 3), (2, 2, 8, 64, 64, 21)]
HEAD_SEEDS = [4, 1]
_CACHE = {}


def random_weights(rng, K1, H1, H2, C):
    """mixed signs; biases of magnitude 0.1 .. 0.5 and kernels scaled so that a layer's product has a spread of about 0.3: most
    pre-activations stay clear of zero (the mask condition) while every column still switches on for some rows and off for others"""
    out = {}
    for name, (fi, fo) in zip(LAYERS, ((K1, H1), (H1, H2), (H2, C), (H2, 4 * C))):
        out[name] = {"kernel": (rng.uniform(-1.0, 1.0, size=(fi, fo)) * 0.5 * np.sqrt(3.0 / fi)).astype(np.float32),
                     "bias": (rng.uniform(0.1, 0.5, size=(fo,)) * rng.choice([-1.0, 1.0], size=(fo,))).astype(np.float32)}
    return out


def head_case(index):
    """weights, pooled (2,37,ph,pw,Cf) and the float64 forward of HEAD_CONFIGS[index], computed once and read-only"""
    if ("head", index) in _CACHE:
        return _CACHE[("head", index)]
    ph, pw, Cf, H1, H2, C = HEAD_CONFIGS[index]
    rng = np.random.RandomState(HEAD_SEEDS[index])
    weights = random_weights(rng, ph * pw * Cf, H1, H2, C)
    pooled = rng.uniform(-1.0, 1.0, size=(2, 37, ph, pw, Cf)).astype(np.float32)
    pooled[rng.uniform(size=pooled.shape) < 0.05] = 0.0
    assert_masks_are_safe(weights, pooled)
    t = rh.target_case(3)                                    # (B, R) = (2, 37): labels in [-1, 21), ignored rows included
    labels = t["labels"] if C == 21 else np.where(t["labels"] > 0, (t["labels"] - 1) % (C - 1) + 1, t["labels"]).astype(np.int32)
    pooled.setflags(write=False)
    case = dict(dims=HEAD_CONFIGS[index], weights=weights, pooled=pooled, ref=det_head_ref(weights, pooled), labels=labels,
                deltas=t["deltas"])
    _CACHE[("head", index)] = case
    return case


E2E_SEED = 1


def e2e_case():
    """feature map (2,6,6,12), the RoIs / valid counts / targets of target case 3 (2 x 37, rows beyond valid), head config 0; pooled is the
    float32 restatement of the pool, which the device matches bit for bit"""
    if "e2e" in _CACHE:
        return _CACHE["e2e"]
    ph, pw, Cf, H1, H2, C = HEAD_CONFIGS[0]
    rng = np.random.RandomState(E2E_SEED)
    t = rh.target_case(3)
    feat = rng.uniform(-1.0, 1.0, size=(2, 6, 6, Cf)).astype(np.float32)
    weights = random_weights(rng, ph * pw * Cf, H1, H2, C)
    rois = np.clip(t["rois"], 0.0, 1.0).astype(np.float32)
    pooled = rp.roi_pool_ref(feat, rois, ph, pw, valid=t["valid"], dtype=np.float32)
    assert_masks_are_safe(weights, pooled)
    labels = np.where(t["labels"] > 0, (t["labels"] - 1) % (C - 1) + 1, t["labels"]).astype(np.int32)
    case = dict(dims=HEAD_CONFIGS[0], feat=feat, weights=weights, rois=rois, valid=t["valid"], pooled=pooled, labels=labels,
                deltas=t["deltas"])
    _CACHE["e2e"] = case
    return case


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------
def test_flatten_order_on_a_hand_made_case():
    """Keras' Flatten of NHWC: feature (i * pw + j) * Cf + c; a head whose layers are selections reads exactly that entry"""
    pooled = np.arange(16, dtype=np.float32).reshape(1, 1, 2, 2, 4) + 1.0
    eye = np.eye(16, dtype=np.float32)
    pick = np.zeros((16, 2), np.float32)
    pick[(1 * 2 + 0) * 4 + 2, 0] = 1.0                        # (i, j, c) = (1, 0, 2)
    pick[(0 * 2 + 1) * 4 + 3, 1] = 1.0                        # (0, 1, 3)
    weights = {"fc1": {"kernel": eye, "bias": np.zeros(16, np.float32)}, "fc2": {"kernel": eye, "bias": np.zeros(16, np.float32)},
               "cls": {"kernel": pick, "bias": np.zeros(2, np.float32)},
               "reg": {"kernel": np.zeros((16, 8), np.float32), "bias": np.zeros(8, np.float32)}}
    f = det_head_ref(weights, pooled)
    assert f["x"].shape == (1, 16)
    for i in range(2):
        for j in range(2):
            for c in range(4):
                assert f["x"][0, (i * 2 + j) * 4 + c] == pooled[0, 0, i, j, c]
    assert f["logits"].tolist() == [[[float(pooled[0, 0, 1, 0, 2]), float(pooled[0, 0, 0, 1, 3])]]]
    assert np.array_equal(f["x"][0], torch.flatten(torch.from_numpy(pooled)[0, 0]).numpy())


@pytest.mark.parametrize("index", range(len(HEAD_CONFIGS)))
def test_restatement_against_torch_float64_autograd(index):
    c = head_case(index)
    rng = np.random.RandomState(3)
    C = c["dims"][5]
    gl, gd = rng.normal(size=(2, 37, C)), rng.normal(size=(2, 37, 4 * C))
    p = {n: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in c["weights"][n].items()} for n in LAYERS}
    x = torch.tensor(np.asarray(c["pooled"], np.float64), requires_grad=True)
    lin = lambda a, n: torch.nn.functional.linear(a, p[n]["kernel"].t(), p[n]["bias"])
    h2 = torch.relu(lin(torch.relu(lin(x.reshape(74, -1), "fc1")), "fc2"))
    logits, deltas = lin(h2, "cls").reshape(2, 37, C), lin(h2, "reg").reshape(2, 37, 4 * C)
    torch.autograd.backward([logits, deltas], [torch.tensor(gl), torch.tensor(gd)])
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert close(c["ref"]["logits"], logits.detach().numpy()) and close(c["ref"]["deltas"], deltas.detach().numpy())
    g, gp = det_head_backward_ref(c["weights"], c["pooled"], gl, gd)
    assert close(gp, x.grad.numpy())
    for n in LAYERS:
        for k in ("kernel", "bias"):
            assert close(g[n][k], p[n][k].grad.numpy()), (n, k)


def test_bound_covers_a_float32_numpy_forward_and_is_not_vacuous():
    """sanity of `bounds` on the CPU: numpy's own float32 products stay inside it, and it is small (under 2e-3 on O(1) outputs after three worst-case layers)"""
    c = head_case(0)
    b = bounds(c["weights"], c["pooled"])
    w = c["weights"]
    x = np.asarray(c["pooled"]).reshape(74, -1)
    h1 = np.maximum(x @ w["fc1"]["kernel"] + w["fc1"]["bias"], np.float32(0))
    h2 = np.maximum(h1 @ w["fc2"]["kernel"] + w["fc2"]["bias"], np.float32(0))
    logits = (h2 @ w["cls"]["kernel"] + w["cls"]["bias"]).reshape(2, 37, -1)
    assert logits.dtype == np.float32
    assert (np.abs(logits - c["ref"]["logits"]) <= b["logits"]).all()
    assert b["logits"].max() < 2e-3 and b["deltas"].max() < 2e-3 and np.abs(c["ref"]["logits"]).max() > 0.3
    assert_masks_are_safe(e2e_case()["weights"], e2e_case()["pooled"])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    assert "typedef struct rpn_det_head rpn_det_head;" in code


def _create(lib, ph=7, pw=7, Cf=512, H1=4096, H2=4096, C=21, max_rows=2400, trainable=1):
    h = L.vp(0)
    return lib.rpn_det_head_create(ph, pw, Cf, H1, H2, C, max_rows, trainable, ctypes.byref(h)), h


def _aligned(nbytes=256):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, L.vp((ctypes.addressof(raw) + 15) & ~15)


def test_argument_validation_precedes_device_use(lib):
    for bad in (dict(ph=0), dict(pw=-1), dict(Cf=510), dict(Cf=0), dict(H1=1022), dict(H2=6), dict(C=1), dict(max_rows=0), dict(trainable=2)):
        st, h = _create(lib, **bad)
        assert st == L.RPN_ERR_INVALID and not h.value, bad
    assert b"rpn_det_head_create" in lib.rpn_last_error()
    assert lib.rpn_det_head_create(7, 7, 512, 64, 64, 21, 8, 1, None) == L.RPN_ERR_INVALID
    # shapes beyond what one launch can grid (65535 tiles of 64 in grid.y) are refused here, not at the first launch
    limit = 65535 * 64
    for bad in (dict(ph=1, pw=1, Cf=limit + 4, H1=64, H2=64), dict(ph=2048, pw=2048, Cf=4, H1=64, H2=64), dict(H1=limit + 4, H2=64),
                dict(H1=64, H2=limit + 4), dict(H1=64, H2=64, max_rows=limit + 1)):
        st, h = _create(lib, **bad)
        assert st == L.RPN_ERR_INVALID and not h.value, bad
    st, h = _create(lib, ph=1, pw=1, Cf=limit, H1=64, H2=64, max_rows=limit)
    assert st == L.RPN_OK
    lib.rpn_det_head_destroy(h)
    st, h = _create(lib, H1=64, H2=64, max_rows=74)
    assert st == L.RPN_OK and h.value
    keep, p = _aligned()
    try:
        fwd = lambda M, keep_, ptr=p: lib.rpn_det_head_forward(h, ptr, M, keep_, p, p, None)
        assert fwd(75, 0) == L.RPN_ERR_INVALID and b"75" in lib.rpn_last_error()            # M > max_rows
        assert fwd(0, 0) == L.RPN_ERR_INVALID
        assert fwd(4, 2) == L.RPN_ERR_INVALID
        assert fwd(4, 0, L.vp(p.value + 4)) == L.RPN_ERR_INVALID and b"aligned" in lib.rpn_last_error()
        assert lib.rpn_det_head_forward(h, None, 4, 0, p, p, None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_forward(h, p, 4, 0, None, p, None) == L.RPN_ERR_INVALID
        # backward before any kept forward; M > max_rows
        assert lib.rpn_det_head_backward(h, p, 4, p, p, p, None) == L.RPN_ERR_INVALID and b"kept forward" in lib.rpn_last_error()
        assert lib.rpn_det_head_backward(h, p, 75, p, p, None, None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_backward(h, p, 4, None, p, None, None) == L.RPN_ERR_INVALID
        # unknown layer names
        buf = (ctypes.c_float * 8)()
        for fn in (lib.rpn_det_head_get_layer, lib.rpn_det_head_get_gradient):
            assert fn(h, b"fc3", buf, buf, None) == L.RPN_ERR_INVALID and b"fc3" in lib.rpn_last_error()
        assert lib.rpn_det_head_set_layer(h, b"rpn_conv", buf, buf) == L.RPN_ERR_INVALID and b"rpn_conv" in lib.rpn_last_error()
        assert lib.rpn_det_head_set_layer(h, b"fc1", None, buf) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_get_layer(h, b"fc1", buf, buf, None) == L.RPN_ERR_INVALID and b"never set" in lib.rpn_last_error()
        assert lib.rpn_det_head_steps(h) == 0
        # unset layers are host state: refused before any device memory is allocated (with or without a device)
        assert fwd(4, 0) == L.RPN_ERR_INVALID and b"set_layer" in lib.rpn_last_error()
        assert lib.rpn_det_head_adam_step(h, 1e-3, 0.9, 0.999, 1e-7, None) == L.RPN_ERR_INVALID and b"set_layer" in lib.rpn_last_error()
    finally:
        lib.rpn_det_head_destroy(h)
    # the inference head keeps nothing and takes no training call
    st, h = _create(lib, H1=64, H2=64, max_rows=74, trainable=0)
    assert st == L.RPN_OK
    try:
        assert lib.rpn_det_head_forward(h, p, 4, 1, p, p, None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_backward(h, p, 4, p, p, None, None) == L.RPN_ERR_INVALID and b"trainable = 0" in lib.rpn_last_error()
        assert lib.rpn_det_head_adam_step(h, 1e-3, 0.9, 0.999, 1e-7, None) == L.RPN_ERR_INVALID
        buf = (ctypes.c_float * 8)()
        assert lib.rpn_det_head_get_gradient(h, b"fc1", buf, buf, None) == L.RPN_ERR_INVALID
    finally:
        lib.rpn_det_head_destroy(h)
    # rpn_fc_forward
    fc = lambda a=p, w=p, M=4, K=32, N=3, ldw=4, relu=1, out=p: lib.rpn_fc_forward(a, w, None, M, K, N, ldw, relu, out, None)
    for bad in (dict(a=None), dict(out=None), dict(M=0), dict(M=65535 * 128 + 1), dict(N=0), dict(K=30), dict(K=0), dict(ldw=3), dict(ldw=0), dict(N=5), dict(relu=2),
                dict(a=L.vp(p.value + 4)), dict(w=L.vp(p.value + 8))):
        assert fc(**bad) == L.RPN_ERR_INVALID, bad
    assert b"rpn_fc_forward" in lib.rpn_last_error()
    del keep


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_compute_calls_fail_loudly_without_a_device(lib):
    st, h = _create(lib, H1=64, H2=64, max_rows=8)
    keep, p = _aligned()
    buf = (ctypes.c_float * (7 * 7 * 512 * 64))()
    try:
        assert lib.rpn_det_head_set_layer(h, b"fc1", buf, buf) == L.RPN_ERR_NO_DEVICE
        # (no layer can be set without a device, so forward and adam_step stop at their own check of that, before the device)
        assert lib.rpn_det_head_forward(h, p, 4, 1, p, p, None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_adam_step(h, 1e-3, 0.9, 0.999, 1e-7, None) == L.RPN_ERR_INVALID
        assert lib.rpn_fc_forward(p, p, None, 4, 32, 3, 4, 1, p, None) == L.RPN_ERR_NO_DEVICE
        assert b"no CPU fallback" in lib.rpn_last_error()
    finally:
        lib.rpn_det_head_destroy(h)
    del keep


def test_memory_bytes_of_the_inference_head_hold_no_training_state(lib):
    """weights: the eight tensors with cls | reg side by side, padded to a multiple of 4 columns; x 4 (gradient, m, v) when trainable.
    workspace of the inference head: the two hidden layers' outputs and nothing else.  These are the forward's SCRATCH -- h1 and h2
    have to live somewhere while a forward runs, and every forward overwrites them -- not kept state: an inference head refuses keep = 1
    and has no backward to keep them for.  (This is how the header reads "trainable = 0 allocates no kept activations".)  A trainable
    head reuses the same two buffers as its kept activations and adds the backward's buffers, never fewer than dz + d_h1 + d_h2."""
    K1, H1, H2, C, R = 7 * 7 * 512, 4096, 1024, 21, 2400
    npad = (5 * C + 3) // 4 * 4
    n = K1 * H1 + H1 + H1 * H2 + H2 + H2 * npad + npad
    a256 = lambda v: (v + 255) & ~255
    got = {}
    for trainable in (0, 1):
        st, h = _create(lib, H1=H1, H2=H2, C=C, max_rows=R, trainable=trainable)
        assert st == L.RPN_OK
        w, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert lib.rpn_det_head_memory_bytes(h, ctypes.byref(w), ctypes.byref(ws)) == L.RPN_OK
        assert lib.rpn_det_head_memory_bytes(h, None, ctypes.byref(ws)) == L.RPN_ERR_INVALID
        got[trainable] = (w.value, ws.value)
        lib.rpn_det_head_destroy(h)
    acts = a256(4 * R * H1) + a256(4 * R * H2)
    assert got[0] == (4 * n, acts)
    assert got[1][0] == 16 * n
    assert got[1][1] >= 2 * acts + a256(4 * R * npad)


def test_python_object_without_a_device():
    from tf_rpn_amd.models import DetectionHead
    from tf_rpn_amd.predictor import Proposer
    head = DetectionHead(21, hidden=(64, 32), max_rois=16, trainable=False)
    assert head.shapes == {"fc1": (25088, 64), "fc2": (64, 32), "cls": (32, 21), "reg": (32, 84)}
    w = head.initial_weights(seed=3)
    limit = np.sqrt(6.0 / (25088 + 64))
    assert w["fc1"]["kernel"].dtype == np.float32 and np.abs(w["fc1"]["kernel"]).max() <= limit
    assert np.abs(w["fc1"]["kernel"]).max() > 0.99 * limit and not w["fc1"]["bias"].any()
    assert np.array_equal(w["reg"]["kernel"], head.initial_weights(seed=3)["reg"]["kernel"])
    assert head.memory_bytes()[0] == 4 * (25088 * 64 + 64 + 64 * 32 + 32 + 32 * 108 + 108)
    with pytest.raises(ValueError):
        DetectionHead(1)
    with pytest.raises(ValueError):
        head.set_weights({n: {"kernel": np.zeros((2, 2)), "bias": np.zeros(2)} for n in LAYERS})
    with pytest.raises(ValueError):
        head(torch.zeros((1, 2, 7, 7, 256)))
    with pytest.raises(ValueError):
        head(torch.zeros((2, 9, 7, 7, 512)))                 # 18 RoIs > max_rois
    assert callable(Proposer.detect)


def test_det_head_kernel_budgets(lib):
    """the forward GEMM keeps its 64 accumulators and staging registers without scratch and fits two workgroups per CU"""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    vgpr, sspill, vspill, scratch, lds, wg = tab["fc_forward_f32_kernel"]
    assert vgpr <= 168 and sspill == 0 and vspill == 0 and scratch == 0 and lds <= 80 * 1024 and wg == 256
    for name in ("pack_pair_grad_kernel", "relu_mask_kernel"):
        assert tab[name][3] == 0 and tab[name][4] == 0
