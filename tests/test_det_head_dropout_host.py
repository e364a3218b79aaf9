"""CPU suite for the detection head's seeded dropout (rpn_det_head_set_dropout, rpn_det_head_dropout_state,
rpn_det_head_set_dropout_calls, rpn_det_head_get_activation, rpn_dropout_forward, models.DetectionHead(dropout=...)): the numpy
restatement of the contract of include/rpn_hip.h ("Dropout") -- Philox4x32-10 on uint64 arithmetic, the threshold rule, the float64
head forward and backward with masks --, the a-priori bounds the GPU tests (tests/test_gpu_det_head_dropout.py) use, and the ABI
checks that need no device.

The bounds.  tests/test_det_head_host.py bounds a product chain in float32 (`product_bound`, `bounds`), tests/test_det_head_x3_host.py
and tests/test_det_head_x3_train_host.py do the same for split float16; U = 2^-24.  Dropout stores, per dropped layer,
a = fl32(relu(z) * fl32(scale)) where kept and +0 where dropped, against the float64 relu(z) * scale with scale = 1 / (1 - rate):
  * relu is 1-Lipschitz, so the error e_z the pre-activation carries arrives as scale * e_z;
  * fl32(scale) is off by at most U scale (one rounding of the double quotient), and the multiplication rounds once more, U on the
    product: two relative roundings, 2 U |relu(z)| scale in all (second-order terms go into the final doubling, as everywhere here);
  * a dropped element is exactly zero on both sides: its error is 0.
So e_a = keep * (scale * e_z + 2 U |relu(z)| scale), and e_a is what the next product takes as its eA.  The backward propagates the
same way: the masked input gradient is d_pre = [a > 0] fl32(d * fl32(scale)), so e_dpre = mask * (scale * e_d + 2 U |d| scale) with
mask = [z > 0] AND keep.  Nothing in these bounds comes from what the kernels return.

The masks.  The backward bound holds where the device's mask [a_stored > 0] equals float64's [z > 0] AND keep.  keep is an integer
function of indices, the same on both sides.  [z > 0] can differ only where |z| is within its forward bound of zero, and only where
the element is KEPT (a dropped element is zero whatever z is).  z2 depends on the dropped h1, so `assert_masks_are_safe_dropout`
re-evaluates the condition on the dropped forward: no pre-activation within its float32 bound of zero at all, and no KEPT
pre-activation within its split-float16 bound of zero (test_det_head_x3_train_host.py notes that a few z1 of these cases lie inside
that wider bound; the committed seeds drop exactly those).  DROP_SEEDS / DROP_CALLS were chosen on the CPU, from the float64
restatement alone, so that this holds for both HEAD_CONFIGS at rate 0.5.
"""
import ctypes
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_host as dh  # noqa: E402
import test_det_head_x3_host as hx  # noqa: E402
import test_det_head_x3_train_host as tr  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from tf_rpn_amd import _lib as L  # noqa: E402

ROOT = dh.ROOT
U = dh.U
LAYERS = dh.LAYERS
NEW_SYMBOLS = ["rpn_det_head_set_dropout", "rpn_det_head_dropout_state", "rpn_det_head_set_dropout_calls", "rpn_det_head_get_activation",
               "rpn_dropout_forward"]
M32 = np.uint64(0xffffffff)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
KNOWN_ANSWERS = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# ---- the generator and the mask ---------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 on uint64 arrays holding 32-bit words: counter (c0, c1, c2, c3), key (k0, k1) -> the four output words"""
    c = [np.asarray(v, np.uint64) & M32 for v in counter]
    k0, k1 = (np.asarray(v, np.uint64) & M32 for v in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]             # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
    return c


def threshold(rate):
    """thr = min(llround(rate 2^32), 2^32 - 1): exact rational arithmetic on the double (round half away from zero, rate >= 0)"""
    return min(int(math.floor(Fraction(float(rate)) * 2 ** 32 + Fraction(1, 2))), 2 ** 32 - 1)


def scale_of(rate):
    """(float)(1.0 / (1.0 - rate)): the double quotient rounded once to float32"""
    return np.float32(1.0 / (1.0 - float(rate)))


def words(seed, calls, layer, M, N):
    """(M, N) uint64: element (m, n)'s word -- output word m & 3 of counter (n, m >> 2, layer, calls mod 2^32), key (seed lo, seed hi)"""
    seed = int(seed) & (2 ** 64 - 1)
    mq, n = np.meshgrid(np.arange((M + 3) // 4, dtype=np.uint64), np.arange(N, dtype=np.uint64), indexing="ij")
    out = philox4x32_10((n, mq, np.full_like(n, layer), np.full_like(n, int(calls) & 0xffffffff)), (seed & 0xffffffff, seed >> 32))
    return np.stack(out, axis=1).reshape(4 * mq.shape[0], N)[:M]


def keep_mask(rate, seed, calls, layer, M, N):
    return words(seed, calls, layer, M, N) >= np.uint64(threshold(rate))


def dropout_ref(x, rate, seed, calls=0, layer=0):
    """rpn_dropout_forward on a float32 (M, N) array, bit for bit: keep ? fl32(x * scale) : +0"""
    x = np.asarray(x, np.float32)
    keep = keep_mask(rate, seed, calls, layer, *x.shape)
    return np.where(keep, x * scale_of(rate), np.float32(0.0)).astype(np.float32)


# ---- the float64 restatement with masks ----------------------------------------------------------------------------------------------------
def head_masks(dims, rate, seed, calls, M=74):
    """(keep1 (M, H1), keep2 (M, H2)) of a kept forward at call number `calls`"""
    H1, H2 = dims[3], dims[4]
    return keep_mask(rate, seed, calls, 0, M, H1), keep_mask(rate, seed, calls, 1, M, H2)


def det_head_ref_dropout(weights, pooled, masks, rate):
    """dh.det_head_ref with h_l = relu(z_l) * scale * keep_l, scale = 1 / (1 - rate) in double"""
    w = dh._w64(weights)
    s = 1.0 / (1.0 - float(rate))
    p = np.asarray(pooled, np.float64)
    B, R = p.shape[:2]
    x = p.reshape(B * R, -1)
    z1 = x @ w["fc1"]["kernel"] + w["fc1"]["bias"]
    h1 = np.maximum(z1, 0.0) * s * masks[0]
    z2 = h1 @ w["fc2"]["kernel"] + w["fc2"]["bias"]
    h2 = np.maximum(z2, 0.0) * s * masks[1]
    logits = h2 @ w["cls"]["kernel"] + w["cls"]["bias"]
    deltas = h2 @ w["reg"]["kernel"] + w["reg"]["bias"]
    return dict(x=x, z1=z1, h1=h1, z2=z2, h2=h2, logits=logits.reshape(B, R, -1), deltas=deltas.reshape(B, R, -1), scale=s)


def det_head_backward_ref_dropout(weights, pooled, masks, rate, grad_logits, grad_deltas):
    """dh.det_head_backward_ref with the masks: d_pre = d * [z > 0] * keep * scale"""
    w = dh._w64(weights)
    f = det_head_ref_dropout(weights, pooled, masks, rate)
    M, s = f["x"].shape[0], f["scale"]
    gl, gd = np.asarray(grad_logits, np.float64).reshape(M, -1), np.asarray(grad_deltas, np.float64).reshape(M, -1)
    g = {"cls": {"kernel": f["h2"].T @ gl, "bias": gl.sum(axis=0)}, "reg": {"kernel": f["h2"].T @ gd, "bias": gd.sum(axis=0)}}
    d2 = (gl @ w["cls"]["kernel"].T + gd @ w["reg"]["kernel"].T) * ((f["z2"] > 0) & masks[1]) * s
    g["fc2"] = {"kernel": f["h1"].T @ d2, "bias": d2.sum(axis=0)}
    d1 = (d2 @ w["fc2"]["kernel"].T) * ((f["z1"] > 0) & masks[0]) * s
    g["fc1"] = {"kernel": f["x"].T @ d1, "bias": d1.sum(axis=0)}
    return g, (d1 @ w["fc1"]["kernel"].T).reshape(np.shape(pooled))


# ---- the a-priori bounds ----------------------------------------------------------------------------------------------------------------
def _products(x3):
    """(forward, wgrad, dgrad) product bounds, undoubled: float32 (dh.product_bound) or split float16 (hx / tr)"""
    if x3:
        return (lambda A, W, b, eA: hx.product_bound_x3(A, W, b, eA=eA, final=False),
                lambda a, ea, dz, edz: tr.wgrad_bound(a, dz, ea=ea, edz=edz, final=False),
                lambda dz, w, edz: tr.dgrad_bound(dz, w, edz=edz, final=False))
    return (lambda A, W, b, eA: dh.product_bound(A, W, b, eA=eA, final=False),
            lambda a, ea, dz, edz: dh.product_bound(a.T, dz, eA=None if ea is None else ea.T, eW=edz, final=False),
            lambda dz, w, edz: dh.product_bound(dz, w.T, eA=edz, final=False))


def dropped_error(value, e_value, keep, scale):
    """module docstring: the error of keep * fl32(value * fl32(scale)) for a float64 `value` carrying e_value -- the carried error
    times scale plus the two relative roundings (scale's own, the multiplication's) on |value| scale; zero where dropped"""
    return keep * (scale * e_value + 2.0 * U * np.abs(value) * scale)


def bounds_dropout(weights, pooled, masks, rate, grad_logits=None, grad_deltas=None, e_grad_logits=None, e_grad_deltas=None, x3=False):
    """dh.bounds (x3: hx.bounds_x3 / tr.bounds_train) for a forward dropped with `masks` at `rate`: "z1", "z2", "h1", "h2" (the
    stored activations against float64 h * scale), "logits", "deltas"; with the output gradients also {layer: {"kernel", "bias"}} and
    "grad_pooled".  Every entry is the doubled total."""
    fwd, wgrad, dgrad = _products(x3)
    w = dh._w64(weights)
    f = det_head_ref_dropout(weights, pooled, masks, rate)
    s = f["scale"]
    B, R = np.shape(pooled)[:2]
    k1, k2 = masks
    e1 = fwd(f["x"], w["fc1"]["kernel"], w["fc1"]["bias"], None)
    eh1 = dropped_error(np.maximum(f["z1"], 0.0), e1, k1, s)
    e2 = fwd(f["h1"], w["fc2"]["kernel"], w["fc2"]["bias"], eh1)
    eh2 = dropped_error(np.maximum(f["z2"], 0.0), e2, k2, s)
    el = fwd(f["h2"], w["cls"]["kernel"], w["cls"]["bias"], eh2)
    ed = fwd(f["h2"], w["reg"]["kernel"], w["reg"]["bias"], eh2)
    out = {"z1": 2 * e1, "z2": 2 * e2, "h1": 2 * eh1, "h2": 2 * eh2, "logits": 2 * el.reshape(B, R, -1), "deltas": 2 * ed.reshape(B, R, -1)}
    if grad_logits is None:
        return out
    M = f["x"].shape[0]
    gl, gd = np.asarray(grad_logits, np.float64).reshape(M, -1), np.asarray(grad_deltas, np.float64).reshape(M, -1)
    C = gl.shape[1]
    egl = np.zeros_like(gl) if e_grad_logits is None else np.asarray(e_grad_logits, np.float64).reshape(M, -1)
    egd = np.zeros_like(gd) if e_grad_deltas is None else np.asarray(e_grad_deltas, np.float64).reshape(M, -1)
    ones = np.ones((1, M))
    bias = lambda d, e: 2 * dh.product_bound(ones, d, eW=e, final=False)[0]         # the bias sums are float32 in both precisions
    dz, edz = np.concatenate([gl, gd], axis=1), np.concatenate([egl, egd], axis=1)
    wp = np.concatenate([w["cls"]["kernel"], w["reg"]["kernel"]], axis=1)          # the pair is ONE product of inner length 5 C
    ep, bp = 2 * wgrad(f["h2"], eh2, dz, edz), bias(dz, edz)
    out["cls"], out["reg"] = {"kernel": ep[:, :C], "bias": bp[:C]}, {"kernel": ep[:, C:], "bias": bp[C:]}
    m2, m1 = (f["z2"] > 0) & k2, (f["z1"] > 0) & k1
    pre2 = dz @ wp.T
    d2 = pre2 * m2 * s
    ed2 = dropped_error(pre2, dgrad(dz, wp, edz), m2, s)
    out["fc2"] = {"kernel": 2 * wgrad(f["h1"], eh1, d2, ed2), "bias": bias(d2, ed2)}
    pre1 = d2 @ w["fc2"]["kernel"].T
    d1 = pre1 * m1 * s
    ed1 = dropped_error(pre1, dgrad(d2, w["fc2"]["kernel"], ed2), m1, s)
    out["fc1"] = {"kernel": 2 * wgrad(f["x"], None, d1, ed1), "bias": bias(d1, ed1)}
    out["grad_pooled"] = 2 * dgrad(d1, w["fc1"]["kernel"], ed1).reshape(np.shape(pooled))
    return out


def assert_masks_are_safe_dropout(weights, pooled, masks, rate):
    """module docstring, "The masks": decided by the float64 restatement alone"""
    f = det_head_ref_dropout(weights, pooled, masks, rate)
    b32, b16 = bounds_dropout(weights, pooled, masks, rate), bounds_dropout(weights, pooled, masks, rate, x3=True)
    for z, keep in (("z1", masks[0]), ("z2", masks[1])):
        near = np.abs(f[z]) <= b32[z]
        assert not near.any(), "%s: %d pre-activations within their float32 bound of zero -- choose another seed" % (z, int(near.sum()))
        near = (np.abs(f[z]) <= b16[z]) & keep
        assert not near.any(), "%s: %d kept pre-activations within their split-float16 bound of zero -- choose another seed" % (z, int(near.sum()))


# ---- cases (built once, read-only) ----------------------------------------------------------------------------------------------------------
RATE = 0.5
DROP_SEEDS = [0x1234567812345697, 7]               # per HEAD_CONFIGS entry; one of them above 2^32 (module docstring, "The masks")
DROP_CALLS = [0, 0]
_CACHE = {}


def drop_case(index):
    """dh.head_case(index) with its dropout seed, call number, masks and the float64 dropped forward at RATE"""
    if index not in _CACHE:
        c = dict(dh.head_case(index))
        c["seed"], c["calls"] = DROP_SEEDS[index], DROP_CALLS[index]
        c["masks"] = head_masks(c["dims"], RATE, c["seed"], c["calls"])
        assert_masks_are_safe_dropout(c["weights"], c["pooled"], c["masks"], RATE)
        c["ref"] = det_head_ref_dropout(c["weights"], c["pooled"], c["masks"], RATE)
        _CACHE[index] = c
    return _CACHE[index]


def edge_rates(seed=3, calls=0, layer=0, m=5, n=7):
    """the edge of the compare: with rate = w / 2^32 (exact in double) element (m, n), whose word is w, is kept; with (w + 1) / 2^32
    it is dropped.  -> (kept rate, dropped rate); the word is asserted to leave room for both"""
    wd = int(words(seed, calls, layer, m + 1, n + 1)[m, n])
    assert 0 < wd < 2 ** 32 - 1
    return wd / 2.0 ** 32, (wd + 1) / 2.0 ** 32


# ---- 1. the generator, the threshold, the mask ------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, expect in KNOWN_ANSWERS:
        assert tuple(int(v) for v in philox4x32_10(counter, key)) == expect
    # vectorised: the three at once
    cs = [np.array([k[0][i] for k in KNOWN_ANSWERS], np.uint64) for i in range(4)]
    ks = [np.array([k[1][i] for k in KNOWN_ANSWERS], np.uint64) for i in range(2)]
    got = philox4x32_10(cs, ks)
    assert [tuple(int(g[j]) for g in got) for j in range(3)] == [k[2] for k in KNOWN_ANSWERS]


def test_threshold_rule():
    assert threshold(0.0) == 0 and threshold(0.5) == 2 ** 31
    assert threshold(0.1) == 429496730                         # 0.1 * 2^32 = 429496729.6...
    assert threshold(2.0 ** -32) == 1 and threshold(2.0 ** -33) == 1 and threshold(2.0 ** -34) == 0     # half rounds away from zero
    assert threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1          # llround gives 2^32: the clamp applies
    assert scale_of(0.0) == 1.0 and scale_of(0.5) == 2.0 and scale_of(1.0 - 2.0 ** -40) == np.float32(2.0 ** 40)
    assert scale_of(0.1) == np.float32(1.0 / 0.9) and scale_of(0.1).dtype == np.float32
    # rate 0 keeps everything (every word is >= 0); the clamped threshold still keeps a word of 2^32 - 1
    assert keep_mask(0.0, 1, 0, 0, 9, 5).all()
    assert np.uint64(0xffffffff) >= np.uint64(threshold(1.0 - 2.0 ** -40))


def test_word_layout_and_the_edge_of_the_compare():
    w = words(0x1234567812345678, 2 ** 32 + 5, 1, 10, 6)         # calls enters mod 2^32
    assert w.shape == (10, 6) and np.array_equal(w, words(0x1234567812345678, 5, 1, 10, 6))
    for m, n in ((0, 0), (3, 5), (4, 0), (9, 2)):
        out = philox4x32_10((n, m >> 2, 1, 5), (0x12345678, 0x12345678))
        assert int(w[m, n]) == int(out[m & 3])
    assert not np.array_equal(w, words(0x1234567812345678, 5, 0, 10, 6))           # the layer is part of the counter
    assert np.array_equal(words(9, 0, 0, 74, 8), words(9, 0, 0, 130, 8)[:74])        # a row's words do not depend on the row count
    kept_rate, dropped_rate = edge_rates()
    x = np.ones((6, 8), np.float32)
    assert dropout_ref(x, kept_rate, 3)[5, 7] == scale_of(kept_rate) and keep_mask(kept_rate, 3, 0, 0, 6, 8)[5, 7]
    assert dropout_ref(x, dropped_rate, 3)[5, 7] == 0.0 and not keep_mask(dropped_rate, 3, 0, 0, 6, 8)[5, 7]
    assert threshold(kept_rate) + 1 == threshold(dropped_rate)


@pytest.mark.parametrize("rate", [0.5, 0.1])
def test_keep_share(rate):
    n = 512 * 512
    p = 1.0 - threshold(rate) / 2.0 ** 32
    for seed, calls, layer in ((DROP_SEEDS[0], 0, 0), (DROP_SEEDS[1], 3, 1)):
        share = keep_mask(rate, seed, calls, layer, 512, 512).mean()
        print("rate %.1f seed %#x: keep share %.6f (expected %.6f, 5 sigma %.6f)" % (rate, seed, share, p, 5 * math.sqrt(p * (1 - p) / n)))
        assert abs(share - p) <= 5 * math.sqrt(p * (1 - p) / n)


# ---- 2. the restatement and the bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_restatement_with_masks_against_torch_float64_autograd(index):
    c = drop_case(index)
    rng = np.random.RandomState(3)
    C = c["dims"][5]
    gl, gd = rng.normal(size=(2, 37, C)), rng.normal(size=(2, 37, 4 * C))
    p = {n: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in c["weights"][n].items()} for n in LAYERS}
    x = torch.tensor(np.asarray(c["pooled"], np.float64), requires_grad=True)
    k1, k2 = (torch.tensor(m.astype(np.float64)) for m in c["masks"])
    s = 1.0 / (1.0 - RATE)
    lin = lambda a, n: torch.nn.functional.linear(a, p[n]["kernel"].t(), p[n]["bias"])
    h1 = torch.relu(lin(x.reshape(74, -1), "fc1")) * s * k1
    h2 = torch.relu(lin(h1, "fc2")) * s * k2
    logits, deltas = lin(h2, "cls").reshape(2, 37, C), lin(h2, "reg").reshape(2, 37, 4 * C)
    torch.autograd.backward([logits, deltas], [torch.tensor(gl), torch.tensor(gd)])
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert close(c["ref"]["logits"], logits.detach().numpy()) and close(c["ref"]["deltas"], deltas.detach().numpy())
    assert close(c["ref"]["h1"], h1.detach().numpy()) and close(c["ref"]["h2"], h2.detach().numpy())
    g, gp = det_head_backward_ref_dropout(c["weights"], c["pooled"], c["masks"], RATE, gl, gd)
    assert close(gp, x.grad.numpy())
    for n in LAYERS:
        for k in ("kernel", "bias"):
            assert close(g[n][k], p[n][k].grad.numpy()), (n, k)
    # with all-ones masks at rate 0 it is dh.det_head_ref
    ones = (np.ones((74, c["dims"][3]), bool), np.ones((74, c["dims"][4]), bool))
    plain = det_head_ref_dropout(c["weights"], c["pooled"], ones, 0.0)
    assert np.array_equal(plain["logits"], dh.head_case(index)["ref"]["logits"])


def float32_forward(c, rate=RATE):
    """the contract in numpy float32: products in float32, a = keep ? fl32(relu(z) * fl32(scale)) : +0"""
    w, s = c["weights"], scale_of(rate)
    x = np.asarray(c["pooled"]).reshape(74, -1)
    h1 = np.where(c["masks"][0], np.maximum(x @ w["fc1"]["kernel"] + w["fc1"]["bias"], np.float32(0)) * s, np.float32(0))
    h2 = np.where(c["masks"][1], np.maximum(h1 @ w["fc2"]["kernel"] + w["fc2"]["bias"], np.float32(0)) * s, np.float32(0))
    logits = (h2 @ w["cls"]["kernel"] + w["cls"]["bias"]).reshape(2, 37, -1)
    assert h1.dtype == np.float32 and h2.dtype == np.float32 and logits.dtype == np.float32
    return h1, h2, logits


def test_bound_covers_a_float32_numpy_forward_and_is_not_vacuous():
    c = drop_case(0)
    b = bounds_dropout(c["weights"], c["pooled"], c["masks"], RATE)
    h1, h2, logits = float32_forward(c)
    for got, name in ((h1, "h1"), (h2, "h2"), (logits, "logits")):
        err = np.abs(got - c["ref"][name])
        print("%s: max err %.3e, max err / bound %.3f" % (name, err.max(), (err / np.maximum(b[name], 1e-300)).max()))
        assert (err <= b[name]).all() and err.max() > 0
    assert not b["h1"][~c["masks"][0]].any() and not b["h2"][~c["masks"][1]].any()          # a dropped element is exact
    assert b["logits"].max() < 4e-3 and b["deltas"].max() < 4e-3 and np.abs(c["ref"]["logits"]).max() > 0.3
    # ... and it notices a forgotten scale, a mask of the wrong layer and a mask of the wrong call
    w = c["weights"]
    x = np.asarray(c["pooled"]).reshape(74, -1)
    unscaled = np.where(c["masks"][0], np.maximum(x @ w["fc1"]["kernel"] + w["fc1"]["bias"], np.float32(0)), np.float32(0))
    assert (np.abs(unscaled - c["ref"]["h1"]) > b["h1"]).any()
    for wrong in (keep_mask(RATE, c["seed"], c["calls"], 1, 74, c["dims"][3]), keep_mask(RATE, c["seed"], c["calls"] + 1, 0, 74, c["dims"][3])):
        other = dict(c, masks=(wrong, c["masks"][1]))
        assert (np.abs(float32_forward(other)[0] - c["ref"]["h1"]) > b["h1"]).any()


def emulate_head_x3_dropout(c, rate=RATE):
    """hx.head_emulation with the dropout of the contract: the hidden activations travel as float32, dropped and scaled"""
    w, s = c["weights"], scale_of(rate)
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)
    x = np.asarray(c["pooled"], np.float32).reshape(74, -1)
    h1 = np.where(c["masks"][0], f32(hx.emulate_x3(x, w["fc1"]["kernel"], w["fc1"]["bias"], relu=True)) * s, np.float32(0))
    h2 = np.where(c["masks"][1], f32(hx.emulate_x3(h1, w["fc2"]["kernel"], w["fc2"]["bias"], relu=True)) * s, np.float32(0))
    logits = hx.emulate_x3(h2, w["cls"]["kernel"], w["cls"]["bias"]).reshape(2, 37, -1)
    deltas = hx.emulate_x3(h2, w["reg"]["kernel"], w["reg"]["bias"]).reshape(2, 37, -1)
    return dict(h1=h1, h2=h2, logits=logits, deltas=deltas)


@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_x3_emulation_lies_inside_the_extended_bound(index):
    c = drop_case(index)
    b = bounds_dropout(c["weights"], c["pooled"], c["masks"], RATE, x3=True)
    e = emulate_head_x3_dropout(c)
    for name in ("h1", "h2", "logits", "deltas"):
        err = np.abs(e[name] - c["ref"][name])
        print("%s: max err %.3e, max err / bound %.3f" % (name, err.max(), (err / np.maximum(b[name], 1e-300)).max()))
        assert (err <= b[name]).all()
    # the zero pattern of the emulation is float64's: dropped or z <= 0
    assert np.array_equal(e["h1"] > 0, c["ref"]["h1"] > 0) and np.array_equal(e["h2"] > 0, c["ref"]["h2"] > 0)


@pytest.mark.parametrize("x3", [False, True])
def test_backward_bound_covers_a_float32_numpy_backward(x3):
    """the backward chain in numpy float32 (a stand-in for either precision's device arithmetic) stays inside the extended bound,
    and a backward without the factor `scale` leaves it"""
    c = drop_case(0)
    w, s = c["weights"], scale_of(RATE)
    gl, gd = tr.cpu_loss_gradients(dict(c, ref=c["ref"]))
    gl64, gd64 = gl.astype(np.float64), gd.astype(np.float64)
    b = bounds_dropout(c["weights"], c["pooled"], c["masks"], RATE, gl64, gd64, x3=x3)
    ref_g, ref_gp = det_head_backward_ref_dropout(c["weights"], c["pooled"], c["masks"], RATE, gl64, gd64)
    h1, h2, _ = float32_forward(c)
    x = np.asarray(c["pooled"]).reshape(74, -1)
    dz = np.concatenate([gl.reshape(74, -1), gd.reshape(74, -1)], axis=1)
    wp = np.concatenate([w["cls"]["kernel"], w["reg"]["kernel"]], axis=1)
    for factor, inside in ((s, True), (np.float32(1.0), False)):
        d2 = np.where(h2 > 0, (dz @ wp.T) * factor, np.float32(0))
        d1 = np.where(h1 > 0, (d2 @ w["fc2"]["kernel"].T) * factor, np.float32(0))
        got = {"fc2": h1.T @ d2, "fc1": x.T @ d1, "grad_pooled": (d1 @ w["fc1"]["kernel"].T).reshape(c["pooled"].shape)}
        assert got["fc1"].dtype == np.float32
        ok = all((np.abs(got[n] - (ref_gp if n == "grad_pooled" else ref_g[n]["kernel"])) <= (b[n] if n == "grad_pooled" else b[n]["kernel"])).all()
                 for n in got)
        assert ok == inside, factor
    assert np.abs(ref_gp).max() > 0 and b["grad_pooled"].max() < 1e-2 * np.abs(ref_gp).max()


def test_masks_are_safe_on_the_dropped_forward():
    for index in range(len(dh.HEAD_CONFIGS)):
        c = drop_case(index)                                     # (asserts it)
        assert_masks_are_safe_dropout(c["weights"], c["pooled"], c["masks"], RATE)
        keep1, keep2 = c["masks"]
        assert 0.4 < keep1.mean() < 0.6 and 0.4 < keep2.mean() < 0.6
        # both kinds of zero occur among the stored activations, and the dropped forward differs from the plain one
        assert ((c["ref"]["z1"] > 0) & ~keep1).any() and ((c["ref"]["z1"] <= 0) & keep1).any()
        assert not np.array_equal(c["ref"]["z2"], dh.head_case(index)["ref"]["z2"])
    assert max(DROP_SEEDS) > 2 ** 32


# ---- 3. ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    assert lib.rpn_abi_version() == 1
    # the contract's constants stand in the header
    for text in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "word >= thr"):
        assert text in header, text


def _state(lib, h):
    rate, seed, calls = ctypes.c_double(-1.0), ctypes.c_ulonglong(99), ctypes.c_ulonglong(99)
    assert lib.rpn_det_head_dropout_state(h, ctypes.byref(rate), ctypes.byref(seed), ctypes.byref(calls)) == L.RPN_OK
    return rate.value, seed.value, calls.value


def test_argument_validation_precedes_device_use(lib):
    st, h = dh._create(lib, H1=64, H2=64, max_rows=74)
    assert st == L.RPN_OK
    keep, p = dh._aligned()
    try:
        assert _state(lib, h) == (0.0, 0, 0)
        for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
            assert lib.rpn_det_head_set_dropout(h, bad, 1) == L.RPN_ERR_INVALID, bad
            assert b"rpn_det_head_set_dropout" in lib.rpn_last_error()
        assert _state(lib, h) == (0.0, 0, 0)
        assert lib.rpn_det_head_set_dropout(None, 0.5, 1) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_set_dropout(h, 0.5, 2 ** 64 - 1) == L.RPN_OK                       # needs no device
        assert _state(lib, h) == (0.5, 2 ** 64 - 1, 0)
        assert lib.rpn_det_head_set_dropout_calls(h, 2 ** 40 + 3) == L.RPN_OK
        assert lib.rpn_det_head_set_dropout(h, 0.25, 7) == L.RPN_OK and _state(lib, h) == (0.25, 7, 2 ** 40 + 3)    # t is left alone
        assert lib.rpn_det_head_set_dropout(h, 0.0, 7) == L.RPN_OK and _state(lib, h) == (0.0, 7, 2 ** 40 + 3)
        rate = ctypes.c_double(0)
        assert lib.rpn_det_head_dropout_state(h, ctypes.byref(rate), None, None) == L.RPN_ERR_INVALID
        # get_activation: names, then the kept forward, all host state
        assert lib.rpn_det_head_get_activation(h, b"cls", p, 4, None) == L.RPN_ERR_INVALID and b"cls" in lib.rpn_last_error()
        assert lib.rpn_det_head_get_activation(h, b"fc3", p, 4, None) == L.RPN_ERR_INVALID and b"fc3" in lib.rpn_last_error()
        assert lib.rpn_det_head_get_activation(h, b"fc1", None, 4, None) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_get_activation(h, None, p, 4, None) == L.RPN_ERR_INVALID
        for name in (b"fc1", b"fc2"):
            assert lib.rpn_det_head_get_activation(h, name, p, 4, None) == L.RPN_ERR_INVALID and b"kept forward" in lib.rpn_last_error()
        assert lib.rpn_det_head_get_activation(h, b"fc1", p, 0, None) == L.RPN_ERR_INVALID
    finally:
        lib.rpn_det_head_destroy(h)
    # a head with trainable = 0 takes no dropout (its state reads as rate 0)
    st, h = dh._create(lib, H1=64, H2=64, max_rows=74, trainable=0)
    assert st == L.RPN_OK
    try:
        assert lib.rpn_det_head_set_dropout(h, 0.5, 1) == L.RPN_ERR_INVALID and b"trainable = 0" in lib.rpn_last_error()
        assert lib.rpn_det_head_set_dropout(h, 0.0, 1) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_set_dropout_calls(h, 3) == L.RPN_ERR_INVALID
        assert _state(lib, h) == (0.0, 0, 0)
    finally:
        lib.rpn_det_head_destroy(h)
    # rpn_dropout_forward
    q = L.vp(p.value + 64)
    fwd = lambda x=p, M=4, N=3, rate=0.5, layer=0, out=q: lib.rpn_dropout_forward(x, M, N, rate, 1, 0, layer, out, None)
    for bad in (dict(x=None), dict(out=None), dict(M=0), dict(N=0), dict(N=-4), dict(rate=-0.5), dict(rate=1.0), dict(rate=float("nan")),
                dict(layer=-1), dict(out=p)):
        assert fwd(**bad) == L.RPN_ERR_INVALID, bad
    assert b"rpn_dropout_forward" in lib.rpn_last_error()
    del keep


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_compute_calls_fail_loudly_without_a_device(lib):
    keep, p = dh._aligned()
    assert lib.rpn_dropout_forward(p, 4, 3, 0.5, 1, 0, 0, L.vp(p.value + 64), None) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()
    del keep


def test_python_object_without_a_device():
    from tf_rpn_amd.models import DetectionHead
    from tf_rpn_amd.models import detection_head
    with pytest.raises(ValueError, match="trainable"):
        DetectionHead(21, hidden=(64, 32), max_rois=16, trainable=False, dropout=0.5)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            DetectionHead(21, hidden=(64, 32), max_rois=16, dropout=bad)
    infer = DetectionHead(21, hidden=(64, 32), max_rois=16, trainable=False, dropout=0.0)
    assert infer.dropout_state() == {"rate": 0.0, "seed": 0, "calls": 0}
    with pytest.raises(ValueError):
        infer.set_dropout(0.5)
    head = DetectionHead(21, hidden=(64, 32), max_rois=16, seed=5, dropout=0.5)
    assert head.dropout_state() == {"rate": 0.5, "seed": 5, "calls": 0}                       # dropout_seed=None: the seed
    assert DetectionHead(21, hidden=(64, 32), max_rois=16, seed=None, dropout=0.5).dropout_state()["seed"] == 0
    assert DetectionHead(21, hidden=(64, 32), max_rois=16, seed=5, dropout_seed=2 ** 63 + 1).dropout_state() == {
        "rate": 0.0, "seed": 2 ** 63 + 1, "calls": 0}
    serial = head._serial
    head.set_dropout(0.25, seed=2 ** 40, calls=17)
    assert head.dropout_state() == {"rate": 0.25, "seed": 2 ** 40, "calls": 17} and head._serial > serial
    serial = head._serial
    head.set_dropout(0.1)                                                                     # seed and calls unchanged
    assert head.dropout_state() == {"rate": 0.1, "seed": 2 ** 40, "calls": 17} and head._serial > serial
    state = head.dropout_state()
    other = DetectionHead(21, hidden=(64, 32), max_rois=16, seed=5)
    other.set_dropout(**state)                                                                # the round trip of a resumed run
    assert other.dropout_state() == state
    with pytest.raises(ValueError):
        head.set_dropout(1.0)
    with pytest.raises(ValueError):
        head.kept_activation("cls")
    with pytest.raises(ValueError):
        detection_head.dropout(np.zeros((2, 2), np.float32), 0.5, 1)
    assert callable(detection_head.dropout)


def test_dropout_kernel_budgets(lib):
    """the dropout variants keep their parents' budgets: the generator's state fits beside the accumulators without scratch"""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    vgpr, sspill, vspill, scratch, lds, wg = tab["fc_forward_f32_dropout_kernel"]
    assert vgpr <= 168 and sspill == 0 and vspill == 0 and scratch == 0 and lds <= 80 * 1024 and wg == 256
    for name in ("fc_forward_x3_dropout_kernel", "fc_dgrad_x3_dropout_kernel"):
        vgpr, sspill, vspill, scratch, lds, wg = tab[name]
        assert vgpr <= 256 and sspill == 0 and vspill == 0 and scratch == 0 and lds <= 80 * 1024 and wg == 256, name
    for name in ("relu_scale_mask_kernel", "dropout_forward_kernel"):
        assert tab[name][1] == 0 and tab[name][2] == 0 and tab[name][3] == 0 and tab[name][4] == 0, name
    # the parents are still there under their names
    for name in ("fc_forward_f32_kernel", "fc_forward_x3_kernel", "fc_dgrad_x3_kernel", "relu_mask_kernel"):
        assert name in tab
