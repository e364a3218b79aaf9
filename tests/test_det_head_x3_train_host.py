"""CPU suite for the detection head TRAINED in split float16 (rpn_det_head_set_train_precision, rpn_fc_wgrad_x3, rpn_fc_dgrad_x3,
models.DetectionHead.compile(precision="f16x3")): the ABI checks that need no device, a numpy emulation of the backward's
arithmetic contract (include/rpn_hip.h) built on tests/test_det_head_x3_host.split16, and the a-priori bounds the GPU tests
(tests/test_gpu_det_head_x3_train.py) use.

The emulation.  An output gradient dZ enters as the split of dZ * 2^t, t = `grad_shift_of(dZ)`: 12 - e clamped to [-116, 100] with
max|dZ| = m 2^e, m in [0.5, 1), NaNs skipped, 0 for an all-zero tensor.
  `emulate_wgrad(a, dz)`:  dW = (a_hi^T z_hi + a_hi^T z_lo + a_lo^T z_hi) 2^-t, a split unscaled (the forward's split of it);
  `emulate_dgrad(dz, w)`:  d_in = (z_hi w_hi^T + z_hi w_lo^T + z_lo w_hi^T) 2^-t 2^-s [h > 0], w (K, N) split as w * 2^s with
                           s = hx.shift_of(w) over the whole matrix this product sees.
The three products and their sum are taken in float64; `parts` switches hi hi, hi lo, lo hi (first factor: a for dW, dZ for d_in).

The bounds (`wgrad_bound`, `dgrad_bound`, `bounds_train`), from the inputs alone, U = 2^-24, against float64.  Each is
tests/test_det_head_host.product_bound with these terms, chained the way dh.bounds chains the backward:
  * unscaled operand (pooled features, activations):      where(x == 0, 0, max(2^-22 |x|, 2^-25));
  * shifted gradient operand (max|x| 2^t lies in [2^11, 2^12), the float16 subnormal half-quantum 2^-25 is 2^-36 max|x| there):
                                                          2^-22 |x| + 2^-36 max|x|;
  * shifted weight operand:                               as hx.product_bound_x3 has it, 2^-22 |w| + max(2^-36 max|w|, 2^-49);
  * accumulation of 3 R float32-accumulated terms:        (3 R + 2) U |A| |B|, R the reduction length -- this REPLACES (R + 2) U;
  * the dropped lo lo term:                               2^-22 |A| |B|;
  * an operand that already carries an error adds it to its own term; the ReLU mask passes an error on where it is 1; the total is
    doubled once.
The ReLU masks.  tests/test_det_head_host asserts that no pre-activation of its cases lies within the FLOAT32 forward bound of
zero; the split forward's bound (hx.bounds_x3) is wider and a few pre-activations of those cases do lie inside it (`uncertain_masks`
counts them from the float64 restatement alone).  There the device's mask may differ from float64's, so the masked gradient may be
the whole unmasked entry or zero where float64 has the other: such an entry's bound is |unmasked entry| + its product bound.

Every case the GPU tests use is built here, once, and the emulation is asserted to lie inside the bound on the CPU.  The head cases
need output gradients; on the CPU they are the float64 restatement of the loss gradients (`cpu_loss_gradients`: softmax cross
entropy over the kept rows, Huber over the positive ones) rounded to float32 -- the GPU test takes the device's own.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_host as dh  # noqa: E402
import test_det_head_x3_host as hx  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from tf_rpn_amd import _lib as L  # noqa: E402

ROOT = dh.ROOT
U = dh.U
LAYERS = dh.LAYERS
F32, BF16X3, F16X3, F32W = 0, 1, 2, 3
NEW_SYMBOLS = ["rpn_det_head_set_train_precision", "rpn_det_head_train_precision", "rpn_fc_wgrad_x3", "rpn_fc_dgrad_x3"]


# ---- the emulation ----------------------------------------------------------------------------------------------------------------------
def grad_shift_of(dz):
    """t = 12 - e clamped to [-116, 100], max|dz| = m 2^e with m in [0.5, 1); NaNs are skipped; 0 for no entry > 0"""
    a = np.abs(np.asarray(dz, np.float32))
    a = a[~np.isnan(a)]
    mx = np.float32(a.max()) if a.size else np.float32(0)
    if not mx > 0:
        return 0
    if np.isinf(mx):
        return -116
    return int(min(100, max(-116, 12 - int(np.frexp(mx)[1]))))


def _scaled_split(x, shift):
    with np.errstate(over="ignore", under="ignore"):
        return hx.split16(np.asarray(x, np.float32) * np.float32(2.0 ** shift))     # a power of two: the float32 product is exact


def emulate_wgrad(a, dz, parts=(1, 1, 1), t=None):
    """the contract's dW = a^T dz for float32 a (M, K), dz (M, N), in float64"""
    t = grad_shift_of(dz) if t is None else t
    ah, al = hx.split16(a)
    zh, zl = _scaled_split(dz, t)
    return (parts[0] * (ah.T @ zh) + parts[1] * (ah.T @ zl) + parts[2] * (al.T @ zh)) * 2.0 ** -t


def emulate_dgrad(dz, w, h=None, parts=(1, 1, 1), t=None):
    """the contract's d_in = dz w^T [h > 0] for float32 dz (M, N), w (K, N), h (M, K), in float64"""
    t = grad_shift_of(dz) if t is None else t
    s = hx.shift_of(w)
    zh, zl = _scaled_split(dz, t)
    wh, wl = _scaled_split(w, s)
    out = (parts[0] * (zh @ wh.T) + parts[1] * (zh @ wl.T) + parts[2] * (zl @ wh.T)) * 2.0 ** -t * 2.0 ** -s
    return out if h is None else out * (np.asarray(h) > 0)


def head_backward_emulation(weights, pooled, grad_logits, grad_deltas):
    """the whole backward under the contract -> ({layer: {"kernel", "bias"}}, grad_pooled); every stored tensor travels as float32"""
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)
    B, R = np.shape(pooled)[:2]
    M = B * R
    C = np.shape(grad_logits)[-1]
    x = np.asarray(pooled, np.float32).reshape(M, -1)
    h1 = f32(hx.emulate_x3(x, weights["fc1"]["kernel"], weights["fc1"]["bias"], relu=True))
    h2 = f32(hx.emulate_x3(h1, weights["fc2"]["kernel"], weights["fc2"]["bias"], relu=True))
    dz = np.concatenate([np.asarray(grad_logits, np.float32).reshape(M, -1), np.asarray(grad_deltas, np.float32).reshape(M, -1)], axis=1)
    wp = np.concatenate([weights["cls"]["kernel"], weights["reg"]["kernel"]], axis=1).astype(np.float32)          # (H2, 5 C)
    gp_, bp_ = emulate_wgrad(h2, dz), dz.astype(np.float64).sum(axis=0)
    g = {"cls": {"kernel": gp_[:, :C], "bias": bp_[:C]}, "reg": {"kernel": gp_[:, C:], "bias": bp_[C:]}}
    d2 = f32(emulate_dgrad(dz, wp, h=h2))
    g["fc2"] = {"kernel": emulate_wgrad(h1, d2), "bias": d2.astype(np.float64).sum(axis=0)}
    d1 = f32(emulate_dgrad(d2, np.asarray(weights["fc2"]["kernel"], np.float32), h=h1))
    g["fc1"] = {"kernel": emulate_wgrad(x, d1), "bias": d1.astype(np.float64).sum(axis=0)}
    return g, emulate_dgrad(d1, np.asarray(weights["fc1"]["kernel"], np.float32)).reshape(np.shape(pooled))


# ---- the a-priori bounds ----------------------------------------------------------------------------------------------------------------
def _e_unscaled(x):
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x == 0, 0.0, np.maximum(2.0 ** -22 * x, 2.0 ** -25))


def _e_gradient(x):
    x = np.abs(np.asarray(x, np.float64))
    return 2.0 ** -22 * x + 2.0 ** -36 * (x.max() if x.size else 0.0)


def _e_weight(w):
    w = np.abs(np.asarray(w, np.float64))
    return 2.0 ** -22 * w + max(2.0 ** -36 * w.max(), 2.0 ** -49)


def _plus(e, extra):
    return e if extra is None else e + np.asarray(extra, np.float64)


def wgrad_bound(a, dz, ea=None, edz=None, final=True):
    """Elementwise bound on |x3(a^T dz) - a^T dz| for float64 a (M, K), dz (M, N); ea / edz: the errors their float32 counterparts
    already carry.  `final`: times 2; inner calls of a chain pass False and double once at the end."""
    a, dz = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(dz, np.float64))
    R = a.shape[0]
    e = dh.product_bound(a.T, dz, eA=_plus(_e_unscaled(a), ea).T, eW=_plus(_e_gradient(dz), edz), final=False)
    ab = a.T @ dz
    e = e + 2 * R * U * ab + 2.0 ** -22 * ab                     # (R + 2) U -> (3 R + 2) U, and the dropped lo lo
    return 2.0 * e if final else e


def dgrad_bound(dz, w, edz=None, final=True):
    """Elementwise bound on |x3(dz w^T) - dz w^T| for float64 dz (M, N), w (K, N) (exact master weights); edz as in wgrad_bound"""
    dz, w = np.abs(np.asarray(dz, np.float64)), np.abs(np.asarray(w, np.float64))
    R = dz.shape[1]
    e = dh.product_bound(dz, w.T, eA=_plus(_e_gradient(dz), edz), eW=_e_weight(w).T, final=False)
    ab = dz @ w.T
    e = e + 2 * R * U * ab + 2.0 ** -22 * ab
    return 2.0 * e if final else e


def uncertain_masks(weights, pooled):
    """{"z1", "z2"}: where a pre-activation lies within its split-forward bound of zero (module docstring), from float64 alone"""
    f, b = dh.det_head_ref(weights, pooled), hx.bounds_x3(weights, pooled)
    return {z: np.abs(f[z]) <= b[z] for z in ("z1", "z2")}


def bounds_train(weights, pooled, grad_logits, grad_deltas, e_grad_logits=None, e_grad_deltas=None):
    """{layer: {"kernel", "bias"}} and "grad_pooled" for a head trained in split float16: dh.bounds' backward chain with the split
    products' bounds and hx.product_bound_x3's forward errors of the activations.  Every entry is the doubled total."""
    w = dh._w64(weights)
    f = dh.det_head_ref(weights, pooled)
    M = f["x"].shape[0]
    e1 = hx.product_bound_x3(f["x"], w["fc1"]["kernel"], w["fc1"]["bias"], final=False)
    e2 = hx.product_bound_x3(f["h1"], w["fc2"]["kernel"], w["fc2"]["bias"], eA=e1, final=False)
    gl, gd = np.asarray(grad_logits, np.float64).reshape(M, -1), np.asarray(grad_deltas, np.float64).reshape(M, -1)
    C = gl.shape[1]
    egl = np.zeros_like(gl) if e_grad_logits is None else np.asarray(e_grad_logits, np.float64).reshape(M, -1)
    egd = np.zeros_like(gd) if e_grad_deltas is None else np.asarray(e_grad_deltas, np.float64).reshape(M, -1)
    ones = np.ones((1, M))
    bias = lambda d, ed: 2 * dh.product_bound(ones, d, eW=ed, final=False)[0]        # dh.bounds' bias bound, the carried error in
    dz, edz = np.concatenate([gl, gd], axis=1), np.concatenate([egl, egd], axis=1)
    wp = np.concatenate([w["cls"]["kernel"], w["reg"]["kernel"]], axis=1)          # (H2, 5 C): the pair is ONE product
    out = {}
    ep, bp = 2 * wgrad_bound(f["h2"], dz, ea=e2, edz=edz, final=False), bias(dz, edz)
    out["cls"], out["reg"] = {"kernel": ep[:, :C], "bias": bp[:C]}, {"kernel": ep[:, C:], "bias": bp[C:]}
    m2, m1 = f["z2"] > 0, f["z1"] > 0
    near = uncertain_masks(weights, pooled)
    masked = lambda full, e, m, u: np.where(u, np.abs(full) + e, e * m)             # (module docstring, "The ReLU masks")
    d2 = (dz @ wp.T) * m2
    ed2 = masked(dz @ wp.T, dgrad_bound(dz, wp, edz=edz, final=False), m2, near["z2"])
    out["fc2"] = {"kernel": 2 * wgrad_bound(f["h1"], d2, ea=e1, edz=ed2, final=False), "bias": bias(d2, ed2)}
    d1 = (d2 @ w["fc2"]["kernel"].T) * m1
    ed1 = masked(d2 @ w["fc2"]["kernel"].T, dgrad_bound(d2, w["fc2"]["kernel"], edz=ed2, final=False), m1, near["z1"])
    out["fc1"] = {"kernel": 2 * wgrad_bound(f["x"], d1, edz=ed1, final=False), "bias": bias(d1, ed1)}
    out["grad_pooled"] = 2 * dgrad_bound(d1, w["fc1"]["kernel"], edz=ed1, final=False).reshape(np.shape(pooled))
    return out


# ---- cases (built once, read-only) ------------------------------------------------------------------------------------------------------
GRAD_SCALES = (1.0, 2.0 ** -20, 1e-7)
WGRAD_M, WGRAD_K, WGRAD_N = (1, 74, 130), (108, 132), (3, 15, 132)          # M is the reduction
DGRAD_M, DGRAD_K, DGRAD_N = (1, 74, 130), (108, 132), (3, 15, 68, 132)      # N is the reduction
EDGE_ROWS = (0, 15, 16, 63, 64, 127, 128, 129)
HEAD_GRAD_SCALES = (1.0, 2.0 ** -20)
_CACHE = {}


def _uniform(rng, shape, zeros=0.03):
    x = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    x[rng.uniform(size=shape) < zeros] = 0.0
    return x


def wgrad_case(K, N):
    """a (130, K) with an all-zero row 1 and dz (130, N), uniform [-1, 1] with 3 % zeros; the first M rows are the case of M"""
    key = ("wgrad", K, N)
    if key not in _CACHE:
        rng = np.random.RandomState(7000 + 10 * K + N)
        a, dz = _uniform(rng, (130, K)), _uniform(rng, (130, N))
        a[1] = 0.0
        _CACHE[key] = hx._frozen(dict(a=a, dz=dz))
    return _CACHE[key]


def dgrad_case(K, N):
    """dz (130, N), w (K, N), h (130, K) (about half of it <= 0).  The contract makes a row's bits a function of that row, w and t,
    and t of the tensor's maximum; so that a row alone and the batch share t, each of EDGE_ROWS holds one entry of the top binade
    [0.5, 1) of the data (column 0) -- which most rows of N >= 15 do anyway, and the rows of N = 3 would not."""
    key = ("dgrad", K, N)
    if key not in _CACHE:
        rng = np.random.RandomState(9000 + 10 * K + N)
        dz, w, h = _uniform(rng, (130, N)), _uniform(rng, (K, N)), rng.uniform(-1.0, 1.0, size=(130, K)).astype(np.float32)
        for m in EDGE_ROWS:
            dz[m, 0] = np.float32(rng.uniform(0.5, 1.0) * rng.choice([-1.0, 1.0]))
        assert all(grad_shift_of(dz[m:m + 1]) == grad_shift_of(dz) for m in EDGE_ROWS)
        _CACHE[key] = hx._frozen(dict(dz=dz, w=w, h=h))
    return _CACHE[key]


def scaled(dz, scale):
    return (np.asarray(dz, np.float32) * np.float32(scale)).astype(np.float32)


def pad_columns(x, fill=7.0):
    return hx.pad_columns(np.asarray(x, np.float32), fill)


def cpu_loss_gradients(c):
    """the float64 restatement of d(reg + cls loss) / d(logits, deltas) of head case c, as float32 (module docstring)"""
    logits, deltas = c["ref"]["logits"], c["ref"]["deltas"]
    B, R, C = logits.shape
    lab = np.asarray(c["labels"]).reshape(-1).astype(np.int64)
    l, d = logits.reshape(B * R, C), deltas.reshape(B * R, C, 4)
    kept, pos = lab >= 0, lab > 0
    n_kept, n_pos = max(1, int(kept.sum())), max(1, int(pos.sum()))
    p = np.exp(l - l.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    gl = np.zeros_like(l)
    gl[kept] = p[kept]
    gl[kept, lab[kept]] -= 1.0
    gl /= n_kept
    gd = np.zeros_like(d)
    target = np.asarray(c["deltas"], np.float64).reshape(B * R, 4)
    diff = d[pos, lab[pos]] - target[pos]
    gd[pos, lab[pos]] = np.clip(diff, -1.0, 1.0) / n_pos
    return gl.reshape(B, R, C).astype(np.float32), gd.reshape(B, R, 4 * C).astype(np.float32)


def _ratio(z, ref, bound):
    return float((np.abs(z - ref) / np.maximum(bound, 1e-300)).max())


# ---- 2. the emulation and the bounds ------------------------------------------------------------------------------------------------------
def test_gradient_shift_rule():
    assert grad_shift_of(np.zeros((3, 3))) == 0 and grad_shift_of(np.array([[np.nan, 0.0]])) == 0
    assert grad_shift_of(np.array([[0.999, np.nan]])) == 12 and grad_shift_of(np.array([[1.0]])) == 11
    assert grad_shift_of(np.array([[-2.5]])) == 10 and grad_shift_of(np.array([[1e-7]])) == 35
    assert grad_shift_of(np.array([[2.0 ** -140]])) == 100                      # clamped
    assert grad_shift_of(np.array([[3e38]])) == -116 and grad_shift_of(np.array([[np.inf]])) == -116
    # every finite float32 lands inside float16's range, its maximum in [2^11, 2^12) unless the upper clamp holds
    for v in (3e38, np.finfo(np.float32).max, 1.0, 1e-7, 2.0 ** -80):
        x = np.float32(v) * np.float32(2.0 ** grad_shift_of(np.array([[v]])))
        assert 2.0 ** 11 <= x < 2.0 ** 12


@pytest.mark.parametrize("K", WGRAD_K)
def test_wgrad_emulation_lies_inside_the_bound(K):
    worst = 0.0
    for N in WGRAD_N:
        c = wgrad_case(K, N)
        for scale in GRAD_SCALES:
            dz = scaled(c["dz"], scale)
            for M in WGRAD_M:
                a64, z64 = c["a"][:M].astype(np.float64), dz[:M].astype(np.float64)
                r = _ratio(emulate_wgrad(c["a"][:M], dz[:M]), a64.T @ z64, wgrad_bound(a64, z64))
                assert r <= 1.0, (K, N, scale, M, r)
                worst = max(worst, r)
    print("wgrad K %d: worst emulation error / bound %.3f" % (K, worst))
    assert 0.0 < worst


@pytest.mark.parametrize("K", DGRAD_K)
def test_dgrad_emulation_lies_inside_the_bound(K):
    worst = 0.0
    for N in DGRAD_N:
        c = dgrad_case(K, N)
        w64 = c["w"].astype(np.float64)
        for scale in GRAD_SCALES:
            dz = scaled(c["dz"], scale)
            for M in DGRAD_M:
                z64 = dz[:M].astype(np.float64)
                for h in (None, c["h"][:M]):
                    ref = z64 @ w64.T * (1.0 if h is None else h > 0)
                    r = _ratio(emulate_dgrad(dz[:M], c["w"], h=h), ref, dgrad_bound(z64, w64))
                    assert r <= 1.0, (K, N, scale, M, r)
                    worst = max(worst, r)
    print("dgrad K %d: worst emulation error / bound %.3f" % (K, worst))
    assert 0.0 < worst


def test_the_bounds_notice_a_dropped_product():
    c = wgrad_case(108, 15)
    a64, z64 = c["a"].astype(np.float64), c["dz"].astype(np.float64)
    for parts in ((1, 0, 1), (1, 1, 0), (0, 1, 1)):
        assert (np.abs(emulate_wgrad(c["a"], c["dz"], parts=parts) - a64.T @ z64) > wgrad_bound(a64, z64)).any(), parts
    c = dgrad_case(108, 15)
    z64, w64 = c["dz"].astype(np.float64), c["w"].astype(np.float64)
    for parts in ((1, 0, 1), (1, 1, 0), (0, 1, 1)):
        assert (np.abs(emulate_dgrad(c["dz"], c["w"], parts=parts) - z64 @ w64.T) > dgrad_bound(z64, w64)).any(), parts


def test_the_bounds_notice_a_missing_gradient_shift():
    """at gradient scale 1e-7 the unshifted split (t = 0) loses the lo halves to float16's subnormals and leaves the bound"""
    c = wgrad_case(108, 15)
    dz = scaled(c["dz"], 1e-7)
    a64, z64 = c["a"].astype(np.float64), dz.astype(np.float64)
    assert grad_shift_of(dz) >= 35
    assert (np.abs(emulate_wgrad(c["a"], dz, t=0) - a64.T @ z64) > wgrad_bound(a64, z64)).any()
    c = dgrad_case(108, 15)
    dz = scaled(c["dz"], 1e-7)
    z64, w64 = dz.astype(np.float64), c["w"].astype(np.float64)
    assert (np.abs(emulate_dgrad(dz, c["w"], t=0) - z64 @ w64.T) > dgrad_bound(z64, w64)).any()


def exact_operands(K):
    """hx.exact_case(K) as the two backward products see it: wgrad(a = A^T, dz = W) and dgrad(dz = A, w = W^T) both equal
    hx.emulate_x3(A, W).  A^T has 33 columns; the product needs a multiple of 4, so three zero columns follow (three zero rows of
    the result)."""
    c = hx.exact_case(K)
    A, W = c["A"], c["W"]
    at = np.zeros((K, (A.shape[0] + 3) // 4 * 4), np.float32)
    at[:, :A.shape[0]] = A.T
    return dict(A=A, W=W, at=at, wt=np.ascontiguousarray(W.T), z=hx.emulate_x3(A, W), rows=A.shape[0])


@pytest.mark.parametrize("K", (32, 108))
def test_exact_case_through_both_backward_products(K):
    c = exact_operands(K)
    A, W = c["A"], c["W"]
    assert grad_shift_of(W) == 10 and grad_shift_of(A) == 10 and hx.shift_of(c["wt"]) == 10      # max |.| is just above 2: t = s = 10
    for x in (A, W):                                             # both scaled splits are exact
        hi, lo = _scaled_split(x, 10)
        assert np.array_equal(hi + lo, x.astype(np.float64) * 1024.0) and np.array_equal(hi, np.round(x.astype(np.float64)) * 1024.0)
    got_w = emulate_wgrad(c["at"], W)
    assert np.array_equal(got_w[:c["rows"]], c["z"]) and not got_w[c["rows"]:].any()
    assert np.array_equal(emulate_dgrad(A, c["wt"]), c["z"])
    assert np.array_equal(c["z"].astype(np.float32).astype(np.float64), c["z"])
    for parts in ((1, 0, 1), (1, 1, 0), (0, 1, 1)):
        assert not np.array_equal(emulate_wgrad(c["at"], W, parts=parts)[:c["rows"]], c["z"])
        assert not np.array_equal(emulate_dgrad(A, c["wt"], parts=parts), c["z"])
    # the scaled partial sums stay exact in float32: integers times 2^-4 (dgrad: both operands carry 2^10) below 2^24
    t = np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)) * 2.0 ** 14
    assert t.max() < 2.0 ** 24


@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_head_backward_emulation_lies_inside_bounds_train(index):
    c = dh.head_case(index)
    near = uncertain_masks(c["weights"], c["pooled"])
    print("head %d: %d of %d pre-activations lie within the split-forward bound of zero" % (index, sum(int(v.sum()) for v in near.values()),
                                                                                           sum(v.size for v in near.values())))
    assert sum(int(v.sum()) for v in near.values()) <= 8           # a handful: the bound stays a statement about the arithmetic
    gl, gd = cpu_loss_gradients(c)
    assert np.abs(gl).max() > 0 and np.abs(gd).max() > 0
    for scale in HEAD_GRAD_SCALES + (1e-7, 1e3):
        gls, gds = scaled(gl, scale), scaled(gd, scale)
        ref_g, ref_gp = dh.det_head_backward_ref(c["weights"], c["pooled"], gls, gds)
        b = bounds_train(c["weights"], c["pooled"], gls, gds)
        g, gp = head_backward_emulation(c["weights"], c["pooled"], gls, gds)
        worst = _ratio(gp, ref_gp, b["grad_pooled"])
        for n in LAYERS:
            for k in ("kernel", "bias"):
                worst = max(worst, _ratio(g[n][k], ref_g[n][k], b[n][k]))
        print("head %d scale %g: worst emulation error / bound %.3f" % (index, scale, worst))
        assert worst <= 1.0
        f32 = dh.bounds(c["weights"], c["pooled"], gls, gds)
        assert (b["fc1"]["kernel"] >= f32["fc1"]["kernel"]).all() and b["fc1"]["kernel"].max() < 1e-2 * scale


# ---- 1. ABI without a device --------------------------------------------------------------------------------------------------------------
def _create(lib, trainable=1, **kw):
    args = dict(ph=7, pw=7, Cf=512, H1=4096, H2=1024, C=21, max_rows=2400)
    args.update(kw)
    h = L.vp(0)
    st = lib.rpn_det_head_create(args["ph"], args["pw"], args["Cf"], args["H1"], args["H2"], args["C"], args["max_rows"], trainable,
                                 ctypes.byref(h))
    assert st == L.RPN_OK and h.value
    return h


def _weights_bytes(lib, h):
    w, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rpn_det_head_memory_bytes(h, ctypes.byref(w), ctypes.byref(ws)) == L.RPN_OK
    return w.value, ws.value


def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    assert "t = 12 - e" in header and "TEST ENTRIES" in header      # the contract text and the entries' standing
    assert lib.rpn_abi_version() == 1


def test_set_train_precision_argument_and_state_checks_need_no_device(lib):
    h = _create(lib, H1=64, H2=64, max_rows=74)
    try:
        assert lib.rpn_det_head_train_precision(h) == F32
        for bad in (-1, 4, 17):
            assert lib.rpn_det_head_set_train_precision(h, bad) == L.RPN_ERR_INVALID
        assert b"rpn_det_head_set_train_precision" in lib.rpn_last_error()
        for unsupported in (BF16X3, F32W):
            assert lib.rpn_det_head_set_train_precision(h, unsupported) == L.RPN_ERR_UNSUPPORTED
        assert lib.rpn_det_head_train_precision(h) == F32
        assert lib.rpn_det_head_set_train_precision(h, F16X3) == L.RPN_OK and lib.rpn_det_head_train_precision(h) == F16X3
        assert lib.rpn_det_head_set_train_precision(h, F32) == L.RPN_OK and lib.rpn_det_head_train_precision(h) == F32
        assert lib.rpn_det_head_set_train_precision(None, F32) == L.RPN_ERR_INVALID
        assert lib.rpn_det_head_train_precision(None) == F32
        # unset layers are still refused before the device, at either precision
        assert lib.rpn_det_head_set_train_precision(h, F16X3) == L.RPN_OK
        keep, p = dh._aligned()
        assert lib.rpn_det_head_forward(h, p, 4, 1, p, p, None) == L.RPN_ERR_INVALID and b"set_layer" in lib.rpn_last_error()
        assert lib.rpn_det_head_backward(h, p, 4, p, p, None, None) == L.RPN_ERR_INVALID and b"kept forward" in lib.rpn_last_error()
        del keep
    finally:
        lib.rpn_det_head_destroy(h)
    h = _create(lib, trainable=0, H1=64, H2=64, max_rows=74)
    try:
        for precision in (9, BF16X3, F32, F16X3):
            assert lib.rpn_det_head_set_train_precision(h, precision) == L.RPN_ERR_INVALID
        assert b"trainable = 0" in lib.rpn_last_error()
    finally:
        lib.rpn_det_head_destroy(h)
    # creating a trainable head in F16X3 stays unsupported
    out = L.vp(0)
    assert lib.rpn_det_head_create_ex(7, 7, 512, 64, 64, 21, 74, 1, F16X3, ctypes.byref(out)) == L.RPN_ERR_UNSUPPORTED and not out.value


def test_memory_bytes_of_a_head_training_in_f16x3(lib):
    """w, g, m, v and the packed image: five times the float32 inference head; going back to float32 keeps the image and says so"""
    n = 25088 * 4096 + 4096 + 4096 * 1024 + 1024 + 1024 * 108 + 108
    infer = _create(lib, trainable=0)
    h = _create(lib)
    try:
        base = _weights_bytes(lib, infer)
        assert base[0] == 4 * n and _weights_bytes(lib, h)[0] == 4 * base[0]
        ws = _weights_bytes(lib, h)[1]
        assert lib.rpn_det_head_set_train_precision(h, F16X3) == L.RPN_OK
        assert _weights_bytes(lib, h) == (5 * base[0], ws)
        assert lib.rpn_det_head_set_train_precision(h, F32) == L.RPN_OK
        assert _weights_bytes(lib, h) == (5 * base[0], ws)
    finally:
        lib.rpn_det_head_destroy(h)
        lib.rpn_det_head_destroy(infer)
    # a K that is no multiple of 32 pads the image's rows: fc2's K = 68 -> 96 rows of 128, the pair's K = 128
    h = _create(lib, ph=3, pw=3, Cf=12, H1=68, H2=128, C=3, max_rows=74)
    try:
        assert lib.rpn_det_head_set_train_precision(h, F16X3) == L.RPN_OK
        n = 108 * 68 + 68 + 68 * 128 + 128 + 128 * 16 + 16
        assert _weights_bytes(lib, h)[0] == 16 * n + 4 * (n + 20 * 68 + 28 * 128)
    finally:
        lib.rpn_det_head_destroy(h)


def test_backward_entries_validate_before_device_use(lib):
    keep, p = dh._aligned()
    odd, half = L.vp(p.value + 4), L.vp(p.value + 2)
    wg = lambda a=p, dz=p, M=4, K=32, N=3, ldz=4, ldo=4, out=p, status=None: lib.rpn_fc_wgrad_x3(a, dz, M, K, N, ldz, ldo, out, status, None)
    for bad in (dict(a=None), dict(dz=None), dict(out=None), dict(M=0), dict(N=0), dict(K=0), dict(K=30), dict(ldz=3), dict(ldz=6),
                dict(ldz=0), dict(N=5), dict(ldo=2), dict(a=odd), dict(dz=odd), dict(out=half), dict(status=half)):
        assert wg(**bad) == L.RPN_ERR_INVALID, bad
    assert b"rpn_fc_wgrad_x3" in lib.rpn_last_error()
    dg = lambda dz=p, w=p, M=4, K=32, N=3, ldz=4, ldw=4, h=None, out=p, status=None: lib.rpn_fc_dgrad_x3(dz, w, M, K, N, ldz, ldw, h, out,
                                                                                                      status, None)
    for bad in (dict(dz=None), dict(w=None), dict(out=None), dict(M=0), dict(M=65535 * 128 + 1), dict(K=0), dict(N=0), dict(ldz=3),
                dict(ldw=6), dict(N=5), dict(dz=odd), dict(w=odd), dict(h=half), dict(out=half), dict(status=half)):
        assert dg(**bad) == L.RPN_ERR_INVALID, bad
    assert b"rpn_fc_dgrad_x3" in lib.rpn_last_error()
    del keep


def test_python_compile_precision_checks():
    from tf_rpn_amd.models import DetectionHead
    head = DetectionHead(21, hidden=(64, 32), max_rois=16, seed=None)
    assert head.precision == "f32" and head.train_precision == "f32"
    for bad in ("bf16x3", "f32w", "fp16", None):
        with pytest.raises(ValueError):
            head.compile(precision=bad)
    assert head.train_precision == "f32"
    base = head.memory_bytes()
    head.compile(learning_rate=1e-3, precision="f16x3")
    assert head.train_precision == "f16x3" and head.precision == "f32" and head.trainable
    assert head.memory_bytes()[0] == base[0] // 4 * 5 and head.memory_bytes()[1] == base[1]
    assert head.status() == {"f16_range": False}
    head.compile(learning_rate=1e-3)
    assert head.train_precision == "f32" and head._opt[0] == 1e-3
    infer = DetectionHead(21, hidden=(64, 32), max_rois=16, trainable=False, seed=None)
    with pytest.raises(ValueError):
        infer.compile(precision="f16x3")
    infer.compile(learning_rate=1e-3)                            # as before: Adam's parameters on an inference head are inert
    assert infer.train_precision == "f32"
    x3 = DetectionHead(21, hidden=(64, 32), max_rois=16, trainable=False, seed=None, precision="f16x3")
    assert x3.train_precision == "f16x3"
    with pytest.raises(ValueError):
        DetectionHead(21, hidden=(64, 32), max_rois=16, precision="f16x3")           # still: construction in f16x3 is the inference head's


def test_backward_x3_kernel_budgets(lib):
    """as tests/test_det_head_host.test_det_head_kernel_budgets: the two new GEMMs keep their 64 accumulator registers, fragments and
    staging without scratch, in 64 KB of LDS and 256 threads"""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    for name in ("fc_wgrad_x3_kernel", "fc_dgrad_x3_kernel"):
        vgpr, sspill, vspill, scratch, lds, wg = tab[name]
        assert vgpr <= 256 and sspill == 0 and vspill == 0 and scratch == 0 and lds <= 64 * 1024 and wg == 256, (name, tab[name])
    assert tab["fc_scales_x3_kernel"][3] == 0 and tab["fc_scales_x3_kernel"][4] == 0
    vgpr, sspill, vspill, scratch, lds, wg = tab["fc_forward_x3_kernel"]                 # its interface changed: the budget did not
    assert sspill == 0 and vspill == 0 and scratch == 0 and lds <= 64 * 1024 and wg == 256
