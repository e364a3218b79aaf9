"""Cases, float64 reference, contract emulation and bounds of the fused MobileNetV2 blocks, one block at a time.  Shared by
tests/test_gpu_mnv2_blocks.py (the kernels on an MI355X) and tests/test_mnv2_blocks_host.py (the bounds proved on the CPU, the case
table classified through rpn_model_ir_launch_info).

Reference.  `block_ref(k, x, weights, dtype)` evaluates block k on its own NHWC input with oracle/conv_oracle.py's `_conv`, `_bn`
and `_correct_pad`: expand 1x1 + BN + ReLU6, zero padding of the EXPANDED tensor (`correct_pad` for stride 2), depthwise 3x3 + BN
+ ReLU6, project 1x1 + BN, the residual where the block has one.  Block 0 (the stem block) is Conv1 behind its own padding + bn_Conv1
+ ReLU6 in place of the expand stage, then expanded_conv's depthwise and projection, reading the images.

Weights.  `weights()` is synthetic_weights("mobilenet_v2", seed 7) with, per block, the BatchNorm behind the expand stage
(bn_Conv1, block_k_expand_BN) rescaled: gamma' = c gamma, beta' = c beta - c q35 with c = 6 / (q90 - q35), where q35 and q90 are the
35 % and 90 % quantiles of that BatchNorm's output z on two 64 x 64 uniform images carried through the blocks below in float64.  Then
z' = c (z - q35): about 35 % of the expanded activations lie at 0, 10 % at 6 and the rest inside (plain He weights on [0, 1] images
never reach 6, and the stem's channels are mostly all-negative or all-positive).  Several folded expand biases of every block are
positive, every projection keeps its non-zero folded bias.  `input_conditions` asserts all of it on the float64 reference of whatever input a test uses.

Bounds (U = 2^-24), never from what the kernels give:
  float32 routes   |got - ref64| <= 4 d32 + 1e-6 max(1, max|ref64|), d32 = the largest deviation of torch-CPU float32 evaluating the
                   same block on the same input (the form of tests/anchor_counts.py)
  f16x3 routes     `x3_bound`: elementwise, from the float64 reference and the weights alone.  All three kernel families
                   (ir_block_x3_kernel, ir_block_hrx3_kernel, pw_x3_kernel) run BOTH 1x1 products as three float16 MFMA products
                   (hi hi + hi lo + lo hi of the input and of the weights times 2^s, s = split_weight_shift of the FOLDED matrix =
                   test_det_head_x3_host.shift_of) and the depthwise in float32; the stem block is float32 throughout.  So
                   e1 = product_bound_x3(x, We, be); ReLU6 is 1-Lipschitz; the depthwise passes e1 on as sum |wd| e1 (zero in the
                   padding) and adds its own (9 + 2) U (sum |wd| |h1| + |bd|); ReLU6; e3 = product_bound_x3(h2, Wp, bp, eA = e2); the
                   residual adds one rounding U (|z3| + |x|); the total is doubled (second-order terms), as in that file.  The
                   library folds BatchNorm in float32 (scale = gamma / sqrtf(var + eps), w * scale, beta - mean * scale) while the
                   reference applies it in float64: 5 U |w| per folded weight and 6 U (|beta| + |mean scale|) per folded bias
                   enter each stage beside the weight-split residue.
                   AND `x3_f32_bound`, a scalar: 4 d + 1e-6 max(1, max|ref64|) with d = the largest deviation from float64 of
                   the CONTRACT evaluated on the CPU with float32 accumulation (`emulate_block(acc32=True)`: torch float32 matrix
                   products of the float16 halves) -- the float32 routes' rule applied to the contract.  Why a second bound: x3_bound
                   must allow one float32 rounding per accumulated term against the whole sum |a||w|, (3 K + 2) U sum |a||w|, which at
                   K = 96 .. 576 is 2^-14 .. 2^-11 of a sum that is itself ~sqrt(K) times the result -- while a dropped cross product
                   is 2^-12 per term with random signs, ~2^-13 sqrt(K) / K of that sum.  On the case inputs the contract with one
                   cross product left out stays at 0.03 .. 1.1 of x3_bound (blocks 7 - 12: below 0.12), so x3_bound alone only sees
                   a missing hi hi (170 .. 3700 times the bound).  x3_f32_bound is 2.3e-5 .. 3.1e-5 on these inputs (outputs up to
                   21; x3_bound: 5e-3 .. 0.13) and a dropped cross product is 48 .. 144 times it, on every block.  Measured on an
                   MI355X: the kernels' error is at most 4.5e-6 = 0.17 of x3_f32_bound and 9.4e-4 of x3_bound.
`emulate_block` restates the arithmetic contract in numpy (split16 / emulate_x3 of tests/test_det_head_x3_host.py, depthwise in
float32); the CPU suite proves that it lies inside both bounds on every block, that it LEAVES x3_f32_bound when any one of the three
products of either GEMM is dropped, and x3_bound when hi hi is.
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fnn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_x3_host as x3h  # noqa: E402
from oracle import conv_oracle as cv  # noqa: E402
from tf_rpn_amd.models._rpn_model import RPNModel, synthetic_weights  # noqa: E402

U = 2.0 ** -24
BLOCKS = cv.MNV2_BLOCKS                 # (block_id, in_ch, expansion, out_ch, stride)
NBLOCKS = len(BLOCKS)
F32_ROUTES = ("ir_block", "ir_block_hr", "stem")


def prefix(k):
    return "expanded_conv_" if k == 0 else "block_%d_" % k


def tensor_name(k):
    """the tensor a fused block writes: its projection's name"""
    return prefix(k) + "project"


def hyper(img):
    return {"img_size": img, "anchor_count": 9}


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def _x3(b3, b45, b6, b7):
    """expected f16x3 forms of one batch size: block 3 (chunk, K-split), blocks 4-5 (route, K-split), block 6 and blocks 7-12 K-split"""
    return {"b3": b3, "b45": b45, "b6": b6, "b7": b7}


# forms: {B: ...}.  f16x3: _x3(...); float32 routes: the kernel of block 3.  The batch sizes are the ones at which a form changes.
CASES = [
    dict(id="f16x3-128-b64", precision="f16x3", img=128, max_batch=64,
         forms={1: _x3((48, 3), ("ir_block_x3", 6), 4, 6), 5: _x3((48, 3), ("ir_block_x3", 6), 4, 6),
                10: _x3((48, 3), ("ir_block_x3", 3), 4, 6), 16: _x3((48, 3), ("ir_block_x3", 2), 4, 6),
                21: _x3((48, 1), ("ir_block_x3", 1), 4, 6), 42: _x3((48, 1), ("ir_block_x3", 1), 2, 3),
                64: _x3((48, 1), ("ir_block_x3", 1), 2, 2)}),
    dict(id="f16x3-128-b96", precision="f16x3", img=128, max_batch=96,
         forms={5: _x3((16, 3), ("ir_block_hrx3", 1), 4, 6), 21: _x3((16, 1), ("ir_block_hrx3", 1), 4, 6),
                81: _x3((16, 1), ("ir_block_hrx3", 1), 1, 1), 96: _x3((16, 1), ("ir_block_hrx3", 1), 1, 1)}),
    # spatial sizes 75, 38, 19, 10: odd and even inputs of the stride-2 blocks, ragged 4 x 8 tiles at every level
    dict(id="f16x3-150-b3", precision="f16x3", img=150, max_batch=3,
         forms={1: _x3((48, 3), ("ir_block_x3", 6), 4, 6), 3: _x3((48, 3), ("ir_block_x3", 3), 4, 6)}),
    # 38, 19, 10, 5
    dict(id="f16x3-75-b2", precision="f16x3", img=75, max_batch=2, forms={2: _x3((48, 3), ("ir_block_x3", 6), 4, 6)}),
    # block 3 at 8, 504 and 512 tiles: both float32 kernels on one handle
    dict(id="f32-128-b64", precision="f32", img=128, max_batch=64, forms={1: "ir_block", 63: "ir_block", 64: "ir_block_hr"}),
    dict(id="f32-150-b3", precision="f32", img=150, max_batch=3, forms={1: "ir_block", 3: "ir_block"}),
    dict(id="bf16x3-128-b2", precision="bf16x3", img=128, max_batch=2, forms={2: "ir_block"}),
]


def case_ids():
    return [c["id"] for c in CASES]


def expected_form(case, k, B):
    """(route, chunk or None, K-split) of block k at B images, from the case table"""
    f = case["forms"][B]
    if k == 0:
        return ("stem", 32, 1)
    if case["precision"] != "f16x3":
        if k in (1, 2):
            return ("ir_block_hr", 16 if k == 1 else 48, 1)
        if k == 3:
            return (f, 16, 1)
        return ("ir_block", 32 if k in (4, 5) else 48, 1)
    if k in (1, 2):
        return ("ir_block_hrx3", 32 if k == 1 else 48, 1)
    if k == 3:
        return ("ir_block_hrx3", f["b3"][0], f["b3"][1])
    if k in (4, 5):
        return (f["b45"][0], 32 if f["b45"][0] == "ir_block_x3" else 48, f["b45"][1])
    if k == 6:
        return ("ir_block_hrx3", 48, f["b6"])
    return ("ir_block_x3", 32, f["b7"])


def tiles_of(img, k, B):
    """4 x 8 output tiles of block k (the stem block: 8 x 16) over B images"""
    n = img
    for kk in range(k + 1):
        if kk == 0 or BLOCKS[kk][4] == 2:
            n = (n + 1) // 2
    return (-(-n // 8) * -(-n // 16) if k == 0 else -(-n // 4) * -(-n // 8)) * B


def form(model, k, B):
    """(route, chunk, K-split) from rpn_model_ir_launch_info; the tile count is checked on the way"""
    info = model.ir_launch_info(tensor_name(k), B)
    assert info["tiles"] == tiles_of(model.img_size, k, B), (k, B, info)
    return info["route"], info["chunk"], info["ksplit"]


# ---- weights and images --------------------------------------------------------------------------------------------------------------
def _images_cpu(B, img):
    return torch.rand((B, img, img, 3), generator=torch.Generator().manual_seed(7000 + img))


@functools.lru_cache(maxsize=4)
def images(B, img):
    """(B, img, img, 3) float32 in [0, 1) on the CPU: the first B of one seeded sequence per image size"""
    return _images_cpu(B, img)


def expand_bn(k):
    return "bn_Conv1" if k == 0 else prefix(k) + "expand_BN"


@functools.lru_cache(maxsize=1)
def weights():
    """module docstring, "Weights"; read-only"""
    w = synthetic_weights("mobilenet_v2", hyper(64), seed=7)
    x = images(2, 64).numpy().astype(np.float64)
    for k in range(NBLOCKS):
        z = block_ref(k, x, w, torch.float64)["z1"]
        q35, q90 = np.quantile(z, (0.35, 0.90))
        c = np.float32(6.0 / (q90 - q35))
        bn = dict(w[expand_bn(k)])
        bn["gamma"] = (bn["gamma"] * c).astype(np.float32)
        bn["beta"] = (bn["beta"] * c - np.float32(c * q35)).astype(np.float32)
        w[expand_bn(k)] = bn
        x = block_ref(k, x, w, torch.float64)["out"]
    return w


def scaled_projection(base, bn_name, factor=2.0 ** 14):
    """`base` with gamma and beta of one projection's BatchNorm times `factor`: its float32 output leaves the float16 range"""
    w = dict(base)
    w[bn_name] = dict(base[bn_name], gamma=(base[bn_name]["gamma"] * np.float32(factor)).astype(np.float32),
                      beta=(base[bn_name]["beta"] * np.float32(factor)).astype(np.float32))
    return w


def make(precision, img, max_batch, w=None):
    model = RPNModel("mobilenet_v2", hyper(img), precision=precision, max_batch=max_batch)
    model.set_weights(weights() if w is None else w)
    return model


# ---- the float64 (and torch float32) reference -------------------------------------------------------------------------------------------
def _nhwc64(t):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.float64).numpy()


def _dw_pad(n, stride):
    return cv._correct_pad(n) if stride == 2 else (1, 1)


def block_ref(k, x_nhwc, w, dtype):
    """block k on its NHWC input in `dtype` -> NHWC float64 numpy {"x", "z1" (expand stage before ReLU6), "h1", "h2", "z3"
    (projection + BN), "out"}"""
    _bid, cin, _t, cout, stride = BLOCKS[k]
    relu6 = lambda t: torch.clamp(t, 0.0, 6.0)
    with torch.no_grad():
        x = cv._t(x_nhwc, dtype).permute(0, 3, 1, 2).contiguous()
        if k == 0:
            ph, pw = cv._correct_pad(x.shape[2]), cv._correct_pad(x.shape[3])
            z1 = cv._bn(cv._conv(Fnn.pad(x, (pw[0], pw[1], ph[0], ph[1])), w["Conv1"]["kernel"], None, stride=2, dtype=dtype),
                        w["bn_Conv1"], dtype)
        else:
            z1 = cv._bn(cv._conv(x, w[prefix(k) + "expand"]["kernel"], None, dtype=dtype), w[prefix(k) + "expand_BN"], dtype)
        h1 = relu6(z1)
        ph, pw = _dw_pad(h1.shape[2], stride), _dw_pad(h1.shape[3], stride)
        d = cv._conv(Fnn.pad(h1, (pw[0], pw[1], ph[0], ph[1])), w[prefix(k) + "depthwise"]["kernel"], None, stride=stride,
                     groups=h1.shape[1], dtype=dtype)
        h2 = relu6(cv._bn(d, w[prefix(k) + "depthwise_BN"], dtype))
        z3 = cv._bn(cv._conv(h2, w[prefix(k) + "project"]["kernel"], None, dtype=dtype), w[prefix(k) + "project_BN"], dtype)
        out = x + z3 if (k != 0 and cin == cout and stride == 1) else z3
        return {"x": _nhwc64(x), "z1": _nhwc64(z1), "h1": _nhwc64(h1), "h2": _nhwc64(h2), "z3": _nhwc64(z3), "out": _nhwc64(out)}


def pointwise_ref(x_nhwc, w, name, dtype):
    """block_13_expand (1x1 + BN + ReLU6) on its NHWC input -> NHWC float64 numpy"""
    with torch.no_grad():
        x = cv._t(x_nhwc, dtype).permute(0, 3, 1, 2).contiguous()
        return _nhwc64(torch.clamp(cv._bn(cv._conv(x, w[name]["kernel"], None, dtype=dtype), w[name + "_BN"], dtype), 0.0, 6.0))


def f32_bound(ref64, ref32):
    return 4.0 * np.abs(ref32 - ref64).max() + 1e-6 * max(1.0, np.abs(ref64).max())


def folded(k, w, dtype):
    """BatchNorm folded as rpn_model_set_layer does (eps 1e-3), every operation in `dtype` -> {"We" (cin, cexp), "be", "Wd" (3, 3,
    cexp), "bd", "Wp" (cexp, cout), "bp"} and, per bias, "|be|" ...: |beta| + |mean scale| (what its rounding error scales with)"""
    out = {}
    for role, conv in (("e", "Conv1" if k == 0 else prefix(k) + "expand"), ("d", prefix(k) + "depthwise"), ("p", prefix(k) + "project")):
        bn = w["bn_Conv1" if conv == "Conv1" else conv + "_BN"]
        g, b, m, v = (np.asarray(bn[key], dtype) for key in ("gamma", "beta", "mean", "var"))
        scale = (g / np.sqrt(v + dtype(cv.BN_EPS))).astype(dtype)
        kern = np.asarray(w[conv]["kernel"], dtype)
        if role == "d":
            W = (kern[:, :, :, 0] * scale).astype(dtype)
        else:
            W = (kern.reshape(-1, kern.shape[3]) * scale).astype(dtype)
        out["W" + role] = W
        out["b" + role] = (b - (m * scale).astype(dtype)).astype(dtype)
        out["|b%s|" % role] = np.abs(b.astype(np.float64)) + np.abs(m.astype(np.float64) * scale.astype(np.float64))
    return out


def input_conditions(k, ref, w, label=""):
    """The conditions on a block's inputs (module docstring), asserted on its float64 reference"""
    h1 = ref["h1"]
    at0, at6 = np.mean(h1 == 0.0), np.mean(h1 == 6.0)
    inside = 1.0 - at0 - at6
    assert min(at0, at6, inside) >= 0.01, (label, k, at0, inside, at6)
    f = folded(k, w, np.float64)
    assert (f["be"] > 0).sum() >= 4, (label, k)          # relu6(bias) != 0 in some channels: a halo filled with it instead of zeros shows
    assert (f["bp"] != 0).all(), (label, k)
    return at0, inside, at6


# ---- the f16x3 bound and the contract's emulation ------------------------------------------------------------------------------------------
FOLD_W, FOLD_B = 5 * U, 6 * U


def _dw_abs(t_nhwc, Wd_abs, stride):
    """sum over the nine taps of |wd| t, zero padded as the depthwise is (float64, NHWC in and out)"""
    t = torch.from_numpy(np.ascontiguousarray(t_nhwc)).permute(0, 3, 1, 2)
    ph, pw = _dw_pad(t.shape[2], stride), _dw_pad(t.shape[3], stride)
    wt = torch.from_numpy(np.ascontiguousarray(Wd_abs)).permute(2, 0, 1)[:, None]          # (C, 1, 3, 3)
    with torch.no_grad():
        y = Fnn.conv2d(Fnn.pad(t, (pw[0], pw[1], ph[0], ph[1])), wt, None, stride=stride, groups=t.shape[1])
    return y.permute(0, 2, 3, 1).numpy()


def x3_bound(k, ref, w):
    """Elementwise bound on |f16x3 block k - ref["out"]| (module docstring); blocks 1 .. 12"""
    assert k >= 1
    _bid, cin, _t, cout, stride = BLOCKS[k]
    f = folded(k, w, np.float64)
    x, h1, h2 = ref["x"], ref["h1"], ref["h2"]
    cexp = h1.shape[3]
    A0 = np.abs(x.reshape(-1, cin))
    e1 = x3h.product_bound_x3(A0, f["We"], f["be"], final=False) + A0 @ (FOLD_W * np.abs(f["We"])) + FOLD_B * f["|be|"]
    e1 = e1.reshape(h1.shape)
    Wd = np.abs(f["Wd"])
    own = _dw_abs(h1, Wd, stride)
    e2 = _dw_abs(e1, Wd, stride) + (11 * U + FOLD_W) * own + 11 * U * np.abs(f["bd"]) + FOLD_B * f["|bd|"]
    A2 = np.abs(h2.reshape(-1, cexp))
    e3 = (x3h.product_bound_x3(A2, f["Wp"], f["bp"], eA=e2.reshape(-1, cexp), final=False) + A2 @ (FOLD_W * np.abs(f["Wp"]))
          + FOLD_B * f["|bp|"])
    e3 = e3.reshape(ref["out"].shape)
    if cin == cout and stride == 1:
        e3 = e3 + U * (np.abs(ref["z3"]) + np.abs(x))
    return 2.0 * e3


def _x3_f32(A, W, bias, parts):
    """emulate_x3's product with every accumulation in float32: three torch-CPU float32 matrix products of the float16 halves (each
    elementary product is exact in float32), added in the kernels' order lo hi, hi lo, hi hi, times 2^-s, + bias"""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    s = x3h.shift_of(W)
    (ah, al), (wh, wl) = x3h.split16(A), x3h.split16(W * np.float32(2.0 ** s))
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    with torch.no_grad():
        c = parts[2] * (t(al) @ t(wh))
        c = c + parts[1] * (t(ah) @ t(wl))
        c = c + parts[0] * (t(ah) @ t(wh))
        z = c * np.float32(2.0 ** -s) + t(np.asarray(bias, np.float32))
    return z.numpy()


def emulate_block(k, x_nhwc, w, parts_e=(1, 1, 1), parts_p=(1, 1, 1), acc32=False):
    """The f16x3 blocks' arithmetic contract on a float32 NHWC input -> float32 NHWC: both 1x1 products as emulate_x3 (`parts_*`
    switches hi hi, hi lo, lo hi of the expand / projection), BatchNorm folded in float32, the depthwise and the residual in float32.
    `acc32`: the products accumulated in float32 too (_x3_f32) instead of exactly."""
    assert k >= 1
    _bid, cin, _t, cout, stride = BLOCKS[k]
    f = folded(k, w, np.float32)
    x = np.asarray(x_nhwc, np.float32)
    N, H, W_, _ = x.shape
    cexp = f["We"].shape[1]
    product = _x3_f32 if acc32 else (lambda A, W, b, parts: x3h.emulate_x3(A, W, b, parts=parts))
    z1 = product(x.reshape(-1, cin), f["We"], f["be"], parts_e)
    h1 = np.clip(z1, 0.0, 6.0).astype(np.float32).reshape(N, H, W_, cexp)
    ph, pw = _dw_pad(H, stride), _dw_pad(W_, stride)
    hp = np.pad(h1, ((0, 0), ph, pw, (0, 0)))                                  # zeros: the expanded tensor outside the image
    OH, OW = (H + sum(ph) - 3) // stride + 1, (W_ + sum(pw) - 3) // stride + 1
    acc = np.zeros((N, OH, OW, cexp), np.float32)
    for r in range(3):
        for s in range(3):
            acc += hp[:, r:r + stride * (OH - 1) + 1:stride, s:s + stride * (OW - 1) + 1:stride, :] * f["Wd"][r, s]
    h2 = np.clip(acc + f["bd"], np.float32(0.0), np.float32(6.0)).astype(np.float32)
    z3 = product(h2.reshape(-1, cexp), f["Wp"], f["bp"], parts_p).astype(np.float32).reshape(N, OH, OW, cout)
    return (z3 + x).astype(np.float32) if (cin == cout and stride == 1) else z3


def x3_f32_bound(k, x_nhwc, ref, w):
    """The second, scalar bound of the f16x3 routes (module docstring): 4 d + 1e-6 max(1, max|ref64|), d = the largest deviation from
    float64 of the contract evaluated with float32 accumulation on the CPU -- the float32 routes' rule, on the contract"""
    d = np.abs(emulate_block(k, x_nhwc, w, acc32=True).astype(np.float64) - ref["out"]).max()
    return 4.0 * d + 1e-6 * max(1.0, np.abs(ref["out"]).max())


@functools.lru_cache(maxsize=4)
def cpu_chain(img, B=1):
    """The blocks' inputs without a GPU: B case images carried through the float64 blocks, each block's input rounded to float32 as
    the library would hand it on -> [float32 NHWC input of block k], k = 0 .. 12"""
    x = images(B, img).numpy()
    xs = []
    for k in range(NBLOCKS):
        xs.append(np.ascontiguousarray(x, dtype=np.float32))
        x = block_ref(k, xs[-1], weights(), torch.float64)["out"]
    return xs


@functools.lru_cache(maxsize=40)
def cpu_block(img, k):
    """(float32 input, float64 reference, x3_bound, x3_f32_bound) of block k >= 1 on cpu_chain(img): computed once, read-only"""
    x, w = cpu_chain(img)[k], weights()
    ref = block_ref(k, x, w, torch.float64)
    return x, ref, x3_bound(k, ref, w), x3_f32_bound(k, x, ref, w)
