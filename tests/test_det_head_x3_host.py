"""CPU suite for the split-float16 inference head (RPN_PRECISION_F16X3: rpn_det_head_create_ex, rpn_det_head_status,
rpn_fc_forward_x3, models.DetectionHead(precision="f16x3")): the ABI checks that need no device, a numpy emulation of the
arithmetic contract of include/rpn_hip.h, and the a-priori bound the GPU tests (tests/test_gpu_det_head_x3.py) use.

The emulation (`emulate_x3`): every float32 input x is hi = f16(x), lo = f16(x - hi) (numpy's astype(float16): round to nearest
even, subnormals kept); every weight the same split of w * 2^s, s = `shift_of(W)` (split_weight_shift's rule, one s per layer);
z = (hi hi + hi lo + lo hi) 2^-s + bias with the three products and their sum in float64.

The bound (`product_bound_x3`, `bounds_x3`), from the inputs alone, U = 2^-24, for z = A W + b against float64.  It is
tests/test_det_head_host.product_bound with the split's terms chained in as that function's eA / eW:
  * accumulation: 3 K float32-accumulated terms, (3 K + 2) U (|A| |W| + |b|) -- this REPLACES product_bound's (K + 2) U term;
  * input split residue: the lo half is rounded to float16, whose subnormal quantum is 2^-24:
    eA = where(A == 0, 0, max(2^-22 |A|, 2^-25));
  * weight split residue under the shift (max|W| 2^s lies in [2^11, 2^12), so the quantum 2^-24 2^-s is at most 2^-35 max|W|, half
    of it 2^-36 max|W|; 2^-49 = 2^-25 2^-24 where the shift is clamped at 24):  eW = 2^-22 |W| + max(2^-36 max|W|, 2^-49);
  * the dropped lo lo term: 2^-22 |A| |W|;
  * an input that already carries an error adds it to eA; ReLU passes an error on; the total is doubled (second-order terms, the
    float32 rounding of the stored hidden activations), as in tests/test_det_head_host.
Every case the GPU tests use is built here, once, and the emulation is asserted to lie inside the bound on the CPU.

The exact case (`exact_case`).  The issue describes inputs a = h + l 2^-12, h in {+-1, +-2}, l in {-3 .. 3}, and wants hi = h and
lo = l 2^-12, so that every product is a multiple of 2^-12 and every partial sum is exact in float32 whatever the order.  Under
round-to-nearest-even that does not hold for every (h, l): float16's spacing is 2^-10 above 1 and 2^-11 below it, so e.g.
1 + 3 2^-12 splits into hi = 1 + 2^-10, lo = -2^-12, and hi hi products then need more than 24 bits.  The case therefore draws l
from {-3 .. 3} AMONG THE VALUES FOR WHICH f16(h + l 2^-12) == h (towards zero: |l| <= 1 at |h| = 1, <= 2 at |h| = 2; away from
zero: <= 2 and <= 3) and asserts that split on the CPU; every l of -3 .. 3 still occurs.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_host as dh  # noqa: E402
from test_det_head_host import lib  # noqa: E402,F401  (fixture)
from tf_rpn_amd import _lib as L  # noqa: E402

ROOT = dh.ROOT
U = dh.U
LAYERS = dh.LAYERS
F32, BF16X3, F16X3, F32W = 0, 1, 2, 3
NEW_SYMBOLS = ["rpn_det_head_create_ex", "rpn_det_head_status", "rpn_det_head_forward_layer", "rpn_fc_forward_x3"]


# ---- the emulation ----------------------------------------------------------------------------------------------------------------------
def shift_of(W):
    """split_weight_shift(kernel, count, true): s = 12 - e clamped to [-100, 24], max|w| = m 2^e with m in [0.5, 1); 0 for no weight > 0"""
    mx = np.float32(np.abs(np.asarray(W, np.float32)).max())
    if not mx > 0:
        return 0
    return int(min(24, max(-100, 12 - int(np.frexp(mx)[1]))))


def split16(x):
    """float32 array -> (hi, lo) as float64: hi = f16(x), lo = f16(x - hi), the subtraction in float32 (it is exact)"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def emulate_x3(A, W, bias=None, relu=False, parts=(1, 1, 1)):
    """the contract's z for float32 A (M, K), W (K, N), bias (N) in float64; `parts` switches hi hi, hi lo, lo hi (all on: the contract)"""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    s = shift_of(W)
    ah, al = split16(A)
    wh, wl = split16(W * np.float32(2.0 ** s))            # a power of two: the float32 product is exact (or the range is left)
    z = (parts[0] * (ah @ wh) + parts[1] * (ah @ wl) + parts[2] * (al @ wh)) * 2.0 ** -s
    if bias is not None:
        z = z + np.asarray(bias, np.float64)
    return np.maximum(z, 0.0) if relu else z


def head_emulation(weights, pooled):
    """the whole head under the contract; the hidden activations travel as float32"""
    B, R = np.shape(pooled)[:2]
    x = np.asarray(pooled, np.float32).reshape(B * R, -1)
    h1 = emulate_x3(x, weights["fc1"]["kernel"], weights["fc1"]["bias"], relu=True).astype(np.float32)
    h2 = emulate_x3(h1, weights["fc2"]["kernel"], weights["fc2"]["bias"], relu=True).astype(np.float32)
    logits = emulate_x3(h2, weights["cls"]["kernel"], weights["cls"]["bias"])
    deltas = emulate_x3(h2, weights["reg"]["kernel"], weights["reg"]["bias"])
    return dict(logits=logits.reshape(B, R, -1), deltas=deltas.reshape(B, R, -1))


# ---- the a-priori bound -----------------------------------------------------------------------------------------------------------------
def product_bound_x3(A, W, bias=None, eA=None, final=True):
    """Elementwise bound on |x3(A W + bias) - (A W + bias)| for float64 A (M, K), W (K, N) (module docstring); eA: the error the
    float32 counterpart of A already carries.  `final`: times 2; inner calls of a chain pass False and double once at the end."""
    A, W = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(W, np.float64))
    K = A.shape[1]
    split_a = np.where(A == 0, 0.0, np.maximum(2.0 ** -22 * A, 2.0 ** -25))
    split_w = 2.0 ** -22 * W + max(2.0 ** -36 * W.max(), 2.0 ** -49)
    e = dh.product_bound(A, W, bias, eA=split_a if eA is None else split_a + np.asarray(eA, np.float64), eW=split_w, final=False)
    # product_bound's accumulation term is (K + 2) U (|A||W| + |b|): make it (3 K + 2) U, and add the dropped lo lo
    ab = A @ W
    e = e + 2 * K * U * (ab + (0.0 if bias is None else np.abs(np.asarray(bias, np.float64)))) + 2.0 ** -22 * ab
    return 2.0 * e if final else e


def bounds_x3(weights, pooled):
    """the bound on "z1", "z2", "logits", "deltas" of the f16x3 head, chained through fc1, ReLU, fc2, ReLU and the pair as dh.bounds does"""
    w = dh._w64(weights)
    f = dh.det_head_ref(weights, pooled)
    B, R = np.shape(pooled)[:2]
    e1 = product_bound_x3(f["x"], w["fc1"]["kernel"], w["fc1"]["bias"], final=False)
    e2 = product_bound_x3(f["h1"], w["fc2"]["kernel"], w["fc2"]["bias"], eA=e1, final=False)
    el = product_bound_x3(f["h2"], w["cls"]["kernel"], w["cls"]["bias"], eA=e2, final=False)
    ed = product_bound_x3(f["h2"], w["reg"]["kernel"], w["reg"]["bias"], eA=e2, final=False)
    return {"z1": 2 * e1, "z2": 2 * e2, "logits": 2 * el.reshape(B, R, -1), "deltas": 2 * ed.reshape(B, R, -1)}


# ---- cases (built once, read-only) ------------------------------------------------------------------------------------------------------
GEMM_K, GEMM_N, GEMM_M = (32, 108, 516), (3, 12, 68, 132), (1, 74, 130)
SHIFT_SCALES = (2.0 ** -20, 2.0 ** 18)
LONG_K = (130, 25088, 132)                                   # M, K, N
_CACHE = {}


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def gemm_case(K, N, M=130, seed=None):
    """the float32 test's data: uniform [-1, 1] with 3 % zeros, an all-zero row 1, a bias; Wp pads W to 4 columns with 7.0"""
    key = ("gemm", K, N, M)
    if key not in _CACHE:
        rng = np.random.RandomState(1000 * K + N if seed is None else seed)
        A = rng.uniform(-1.0, 1.0, size=(M, K)).astype(np.float32)
        A[rng.uniform(size=A.shape) < 0.03] = 0.0
        A[1] = 0.0
        W = rng.uniform(-1.0, 1.0, size=(K, N)).astype(np.float32)
        W[rng.uniform(size=W.shape) < 0.03] = 0.0
        bias = rng.uniform(-1.0, 1.0, size=(N,)).astype(np.float32)
        _CACHE[key] = _frozen(dict(A=A, W=W, bias=bias))
    return _CACHE[key]


def pad_columns(W, fill=7.0):
    K, N = W.shape
    Wp = np.full((K, (N + 3) // 4 * 4), fill, np.float32)
    Wp[:, :N] = W
    return Wp


def exact_case(K, M=33, N=20):
    """module docstring: a = h + l 2^-12 with hi = h and lo = l 2^-12, weights of the same form; every l of -3 .. 3 occurs"""
    key = ("exact", K)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.RandomState(77 + K)

    def draw(shape):
        h = rng.choice([-2.0, -1.0, 1.0, 2.0], size=shape)
        away = rng.uniform(size=shape) < 0.5                    # l on the side away from zero
        top = np.where(np.abs(h) == 1, np.where(away, 2, 1), np.where(away, 3, 2))
        l = np.floor(rng.uniform(size=shape) * (top + 1)).astype(np.int64)          # 0 .. top
        l = np.where(away, l, -l) * np.sign(h).astype(np.int64)
        x = (h + l * 2.0 ** -12).astype(np.float32)
        assert np.array_equal(x.astype(np.float64), h + l * 2.0 ** -12)
        return x, h, l

    A, ha, la = draw((M, K))
    W, hw, lw = draw((K, N))
    assert set(np.unique(la)) == set(range(-3, 4)) and set(np.unique(lw)) == set(range(-3, 4))
    hi, lo = split16(A)
    assert np.array_equal(hi, ha) and np.array_equal(lo, la * 2.0 ** -12)
    assert shift_of(W) == 10                                   # max|w| is just above 2: the rule gives s = 10
    hi, lo = split16(W * np.float32(1024.0))
    assert np.array_equal(hi, hw * 1024.0) and np.array_equal(lo, lw * 0.25)
    _CACHE[key] = _frozen(dict(A=A, W=W))
    return _CACHE[key]


def long_k_case():
    if "long" not in _CACHE:
        M, K, N = LONG_K
        rng = np.random.RandomState(5)
        A = rng.uniform(-1.0, 1.0, size=(M, K)).astype(np.float32)
        A[rng.uniform(size=A.shape) < 0.03] = 0.0
        W = (rng.uniform(-1.0, 1.0, size=(K, N)) * np.sqrt(3.0 / K)).astype(np.float32)
        bias = rng.uniform(-1.0, 1.0, size=(N,)).astype(np.float32)
        A64, W64 = A.astype(np.float64), W.astype(np.float64)
        _CACHE["long"] = _frozen(dict(A=A, W=W, bias=bias, ref=A64 @ W64 + bias, bound=product_bound_x3(A64, W64, bias)))
    return _CACHE["long"]


def _inside(z, ref, bound, what):
    err = np.abs(z - ref)
    assert (err <= bound).all(), "%s: the emulation leaves the bound, max err / bound %.3f" % (what, (err / np.maximum(bound, 1e-300)).max())
    return float((err / np.maximum(bound, 1e-300)).max())


# ---- 2. the emulation and the bound -------------------------------------------------------------------------------------------------------
def test_shift_rule_and_split():
    assert shift_of(np.zeros((4, 4))) == 0
    assert shift_of(np.array([[0.999]])) == 12 and shift_of(np.array([[1.0]])) == 11 and shift_of(np.array([[-2.5]])) == 10
    assert shift_of(np.array([[2.0 ** -30]])) == 24 and shift_of(np.array([[2.0 ** 120]])) == -100
    hi, lo = split16(np.array([1.0 + 3 * 2.0 ** -12, 65504.0, 2.0 ** -20, 0.1], np.float32))
    assert hi[0] == 1.0 + 2.0 ** -10 and lo[0] == -2.0 ** -12
    assert hi[1] == 65504.0 and lo[1] == 0.0
    assert hi[2] == 2.0 ** -20 and lo[2] == 0.0                  # a float16 subnormal is kept
    assert abs(hi[3] + lo[3] - np.float32(0.1)) <= 2.0 ** -22 * 0.1
    assert not np.isfinite(split16(np.array([70000.0], np.float32))[0][0])


@pytest.mark.parametrize("K", GEMM_K)
def test_emulation_lies_inside_the_bound_on_the_gemm_grid(K):
    worst = 0.0
    for N in GEMM_N:
        c = gemm_case(K, N)
        A64, b64 = c["A"].astype(np.float64), c["bias"].astype(np.float64)
        for scale in (1.0,) + SHIFT_SCALES:
            W = (c["W"] * np.float32(scale)).astype(np.float32)
            W64 = W.astype(np.float64)
            for use_bias in (False, True):
                ref = A64 @ W64 + (b64 if use_bias else 0.0)
                bound = product_bound_x3(A64, W64, c["bias"] if use_bias else None)
                z = emulate_x3(c["A"], W, c["bias"] if use_bias else None)
                worst = max(worst, _inside(z, ref, bound, "K %d N %d scale %g bias %d" % (K, N, scale, use_bias)))
    print("K %d: worst emulation error / bound %.3f" % (K, worst))
    assert worst > 0.0


def test_emulation_needs_all_three_products():
    """the bound is tight enough to notice a dropped cross product"""
    c = gemm_case(108, 12)
    A64, W64 = c["A"].astype(np.float64), c["W"].astype(np.float64)
    bound = product_bound_x3(A64, W64)
    for parts in ((1, 0, 1), (1, 1, 0), (0, 1, 1)):
        assert (np.abs(emulate_x3(c["A"], c["W"], parts=parts) - A64 @ W64) > bound).any(), parts


@pytest.mark.parametrize("K", (32, 108))
def test_exact_case_is_exact(K):
    c = exact_case(K)
    for scale in (1.0, 2.0 ** 18):
        W = (c["W"] * np.float32(scale)).astype(np.float32)
        z = emulate_x3(c["A"], W) / scale
        t = z * 2.0 ** 14
        assert np.array_equal(t, np.round(t)) and np.abs(t).max() < 2.0 ** 21
        assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
        full = c["A"].astype(np.float64) @ c["W"].astype(np.float64)                 # with lo lo
        assert (full.astype(np.float32) != z.astype(np.float32)).any()               # ... which float32 arithmetic would show
        for parts in ((1, 0, 1), (1, 1, 0), (0, 1, 1)):
            assert not np.array_equal(emulate_x3(c["A"], W, parts=parts) / scale, z)
    A64, W64 = c["A"].astype(np.float64), c["W"].astype(np.float64)
    _inside(emulate_x3(c["A"], c["W"]), A64 @ W64, product_bound_x3(A64, W64), "exact case")


def test_emulation_lies_inside_the_bound_at_long_k():
    c = long_k_case()
    r = _inside(emulate_x3(c["A"], c["W"], c["bias"]), c["ref"], c["bound"], "long K")
    # (3 K + 2) U is 4.5e-3 here: a worst-case statement about 75 264 accumulated terms, far above what any order of summation gives
    print("long K: emulation error / bound %.3e, max bound %.3e" % (r, c["bound"].max()))


@pytest.mark.parametrize("index", range(len(dh.HEAD_CONFIGS)))
def test_head_emulation_lies_inside_bounds_x3(index):
    c = dh.head_case(index)
    b = bounds_x3(c["weights"], c["pooled"])
    e = head_emulation(c["weights"], c["pooled"])
    for k in ("logits", "deltas"):
        _inside(e[k], c["ref"][k], b[k], k)
        assert (b[k] >= dh.bounds(c["weights"], c["pooled"])[k]).all() and b[k].max() < 1e-2


# ---- 1. ABI without a device --------------------------------------------------------------------------------------------------------------
def _create_ex(lib, ph=7, pw=7, Cf=512, H1=4096, H2=4096, C=21, max_rows=2400, trainable=0, precision=F16X3):
    h = L.vp(0)
    return lib.rpn_det_head_create_ex(ph, pw, Cf, H1, H2, C, max_rows, trainable, precision, ctypes.byref(h)), h


def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    assert lib.rpn_abi_version() == 1


def test_create_ex_argument_validation(lib):
    for bad in (dict(ph=0), dict(Cf=510), dict(H1=1022), dict(H2=6), dict(C=1), dict(max_rows=0), dict(trainable=2), dict(precision=4),
                dict(precision=-1)):
        st, h = _create_ex(lib, **bad)
        assert st == L.RPN_ERR_INVALID and not h.value, bad
    assert b"rpn_det_head_create" in lib.rpn_last_error()
    assert lib.rpn_det_head_create_ex(7, 7, 512, 64, 64, 21, 8, 0, F16X3, None) == L.RPN_ERR_INVALID
    for bad in (dict(precision=BF16X3), dict(precision=F32W), dict(precision=BF16X3, trainable=1), dict(trainable=1)):
        st, h = _create_ex(lib, **bad)
        assert st == L.RPN_ERR_UNSUPPORTED and not h.value, bad
        assert b"rpn_det_head_create" in lib.rpn_last_error()
    assert b"float32" in lib.rpn_last_error()                   # F16X3 with trainable = 1: training stays exact float32
    # an invalid argument is reported as such even beside an unsupported precision
    assert _create_ex(lib, Cf=510, precision=BF16X3)[0] == L.RPN_ERR_INVALID
    for trainable in (0, 1):                                    # F32 through _ex is rpn_det_head_create
        st, h = _create_ex(lib, H1=64, H2=64, trainable=trainable, precision=F32)
        assert st == L.RPN_OK and h.value
        lib.rpn_det_head_destroy(h)


def test_f16x3_head_takes_no_training_call_and_reports_no_flag_before_a_forward(lib):
    keep, p = dh._aligned()
    buf = (ctypes.c_float * 8)()
    flags = ctypes.c_uint(7)
    for precision in (F16X3, F32):
        st, h = _create_ex(lib, H1=64, H2=64, max_rows=74, precision=precision)
        assert st == L.RPN_OK and h.value
        try:
            assert lib.rpn_det_head_forward(h, p, 4, 1, p, p, None) == L.RPN_ERR_INVALID
            assert lib.rpn_det_head_backward(h, p, 4, p, p, None, None) == L.RPN_ERR_INVALID and b"trainable = 0" in lib.rpn_last_error()
            assert lib.rpn_det_head_adam_step(h, 1e-3, 0.9, 0.999, 1e-7, None) == L.RPN_ERR_INVALID
            assert lib.rpn_det_head_get_gradient(h, b"fc1", buf, buf, None) == L.RPN_ERR_INVALID
            assert lib.rpn_det_head_forward(h, p, 4, 0, p, p, None) == L.RPN_ERR_INVALID and b"set_layer" in lib.rpn_last_error()
            assert lib.rpn_det_head_forward(h, p, 75, 0, p, p, None) == L.RPN_ERR_INVALID
            flags.value = 7
            assert lib.rpn_det_head_status(h, ctypes.byref(flags), 1, None) == L.RPN_OK and flags.value == 0
            assert lib.rpn_det_head_status(h, None, 0, None) == L.RPN_ERR_INVALID
            assert lib.rpn_det_head_status(None, ctypes.byref(flags), 0, None) == L.RPN_ERR_INVALID
            layer = lambda name=b"fc1", src=p, M=4, dst=p: lib.rpn_det_head_forward_layer(h, name, src, M, dst, None)
            for bad in (dict(name=b"cls"), dict(name=b"fc3"), dict(name=None), dict(src=None), dict(dst=None), dict(M=0),
                        dict(src=L.vp(p.value + 4))):
                assert layer(**bad) == L.RPN_ERR_INVALID, bad
            assert layer() == L.RPN_ERR_INVALID and b"never set" in lib.rpn_last_error()
        finally:
            lib.rpn_det_head_destroy(h)
    del keep


def test_memory_bytes_of_the_f16x3_head(lib):
    """the float32 weights and their packed image of the same size: exactly twice the float32 inference head; the same workspace"""
    got = {}
    for precision in (F32, F16X3):
        st, h = _create_ex(lib, H1=4096, H2=1024, precision=precision)
        assert st == L.RPN_OK
        w, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert lib.rpn_det_head_memory_bytes(h, ctypes.byref(w), ctypes.byref(ws)) == L.RPN_OK
        got[precision] = (w.value, ws.value)
        lib.rpn_det_head_destroy(h)
    n = 25088 * 4096 + 4096 + 4096 * 1024 + 1024 + 1024 * 108 + 108
    assert got[F32][0] == 4 * n and got[F16X3][0] == 2 * got[F32][0] and got[F16X3][1] == got[F32][1]
    # a K that is no multiple of 32 pads the image's rows: 108 -> 128 rows of 68 columns
    st, h = _create_ex(lib, ph=3, pw=3, Cf=12, H1=68, H2=128, C=3, max_rows=74)
    w, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert st == L.RPN_OK and lib.rpn_det_head_memory_bytes(h, ctypes.byref(w), ctypes.byref(ws)) == L.RPN_OK
    n = 108 * 68 + 68 + 68 * 128 + 128 + 128 * 16 + 16
    assert w.value == 4 * n + 4 * (n + 20 * 68 + 28 * 128)      # fc2's K = 68 -> 96 rows
    lib.rpn_det_head_destroy(h)


def test_fc_forward_x3_argument_validation_precedes_device_use(lib):
    keep, p = dh._aligned()
    fc = lambda a=p, w=p, M=4, K=32, N=3, ldw=4, relu=1, out=p, status=None: lib.rpn_fc_forward_x3(a, w, None, M, K, N, ldw, relu, out,
                                                                                                 status, None)
    for bad in (dict(a=None), dict(w=None), dict(out=None), dict(M=0), dict(M=65535 * 128 + 1), dict(N=0), dict(K=30), dict(K=0),
                dict(ldw=3), dict(ldw=0), dict(N=5), dict(relu=2), dict(a=L.vp(p.value + 4)), dict(w=L.vp(p.value + 8)),
                dict(status=L.vp(p.value + 2))):
        assert fc(**bad) == L.RPN_ERR_INVALID, bad
    assert b"rpn_fc_forward_x3" in lib.rpn_last_error()
    del keep


def test_python_object_argument_checks():
    from tf_rpn_amd.models import DetectionHead
    for bad in (dict(precision="bf16x3"), dict(precision="f32w"), dict(precision="fp16"), dict(precision=None),
                dict(precision="f16x3", trainable=True), dict(precision="f16x3")):          # (trainable defaults to True)
        with pytest.raises(ValueError):
            DetectionHead(21, hidden=(64, 32), max_rois=16, **bad)
    head = DetectionHead(21, hidden=(64, 32), max_rois=16, trainable=False, precision="f16x3", seed=None)
    f32 = DetectionHead(21, hidden=(64, 32), max_rois=16, trainable=False, seed=None)
    assert head.precision == "f16x3" and f32.precision == "f32" and not head.trainable
    assert head.memory_bytes() == (2 * f32.memory_bytes()[0], f32.memory_bytes()[1])
    assert head.status() == {"f16_range": False} and f32.status(reset=True) == {"f16_range": False}
    with pytest.raises(ValueError):
        f32.inference_copy(precision="bf16x3")


def test_x3_kernel_budgets(lib):
    """the split GEMM keeps its 64 accumulator registers and fragments without scratch, two workgroups of four waves per CU"""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    vgpr, sspill, vspill, scratch, lds, wg = tab["fc_forward_x3_kernel"]
    assert vgpr <= 256 and sspill == 0 and vspill == 0 and scratch == 0 and lds <= 80 * 1024 and wg == 256
    for name in ("fc_pack_x3_kernel", "fc_absmax_kernel"):
        assert tab[name][3] == 0 and tab[name][4] == 0
