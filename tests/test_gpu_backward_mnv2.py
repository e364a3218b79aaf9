"""The MobileNetV2 backward kernels, one layer at a time, through the public single-layer entries (rpn_batchnorm_train_forward /
_backward, rpn_conv1x1_wgrad / _dgrad, rpn_dwconv3x3_dgrad / _wgrad, rpn_dwconv3x3_s2_dgrad / _s2_wgrad, rpn_conv3x3_s2_cin3_wgrad):
the counterpart of tests/test_gpu_backward.py, built from its parts (Band, settle, same_bytes, the parity bound and MARGIN).

References: float64 numpy restatements of the formulas in include/rpn_hip.h (bn64, conv1x1_64, dw64, dw_s2_64, stem_wgrad64) and,
as a second oracle written independently of them, torch float64 on the CPU (F.batch_norm(training=True) + hardtanh, autograd
through F.conv2d with groups = C, F.pad(x, (pl, 1, pt, 1)) + a stride-2 'valid' conv); test_references_agree_* hold the two against
each other to 1e-13 without a GPU.  torch refuses BatchNorm in training mode over one pixel, so P = 1 rests on the restatement
alone, whose values there are known in closed form (mean = x, var = 0, y = beta, dx = 0, dgamma = 0, dbeta = dy').

Guard bands: every input, output and workspace is a Band (4096 words of NaN canary on both sides; the workspace exactly
*_workspace_bytes long and itself full of canary).  The BatchNorm workspace holds float64 partial sums, and two words of the usual
canary 0x7FC0BEEF read as one float64 are the finite number 2.35e307, so that workspace is filled with 0x7FF8BEEF, a NaN in both
views (test_canaries_are_nan_in_every_view).  Every call runs twice into fresh output and workspace bands (same bytes), and the
input bands are byte-identical before and after.

Bounds on real values: the two of test_gpu_backward.py -- err(gpu) <= margin * max(e32, 2^-24) with e32 the error of a plain
float32 evaluation on the CPU (the *_32 functions), and element-wise |t - ref64| <= (n + depth) 2^-24 (|A| . |B|) with the last
factor the same restatement on absolute values.  BatchNorm keeps the bound of test_train_mobilenet.py: 4 x the largest deviation
of torch float32 from torch float64 over all outputs (numpy float32 at P = 1).
"""
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402
from test_gpu_backward import MARGIN, U, Band, dy_like, same_bytes, settle, workspace  # noqa: E402
from test_train_mobilenet import BN_EPS, BN_MOMENTUM, MOM32, ONE_MINUS_MOM32, bn_torch, ints  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402

TF = torch.nn.functional
CANARY = 0x7FC0BEEF             # test_gpu_backward.py's: a NaN as float32, but two of them are a finite float64
CANARY64 = 0x7FF8BEEF           # a NaN as float32 and, doubled, as float64: for the BatchNorm workspace
EPS32 = float(np.float32(BN_EPS))          # what the kernel receives


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


# ---- shape tables (test_shape_tables_reach_every_path classifies them with the library's own host functions) -------------------------
# Summation-order ratios beside each table: the experiment behind MARGIN (see its comment in test_gpu_backward.py) redone on the CPU
# with this file's data builders and these shapes -- a float32 fma chain in the order the header describes (fixed pixel ranges, a
# chain inside each, the ranges in a pairwise tree) against the *_32 yardstick, both against float64, as chain / max(e32, 2^-24),
# worst of 8 seeds, the worst shape of each table (DESIGN.md 6e has every shape):
#   1x1 dw 1.01 (130, 144, 24)   1x1 dx 4.67 (63, 16, 96); 2.36 at K = 1028, 1.91 at K = 576, 1.00 at K = 4 .. 144 otherwise
#   depthwise dx 1.23 (2, 3, 5, 24)   dw 1.59 (same)      stride 2: dx 1.00, dw 1.77 (2, 10, 10, 40)      stem dw 1.90 (1, 6, 5, 40)
# The long weight-gradient sums come out BELOW 1 (0.07 .. 0.9 from 500 pixels up): the yardsticks of the per-channel entries add
# pixel after pixel, so they lose more than a chain cut into 32 .. 256 leaves does.  None of the ratios exceeds 16 (the largest is
# 4.67), so every entry keeps MARGIN.
# (P, C), each with relu6 0 and 1
BN = [(1, 4),               # the Bessel branch (P > 1 ? ... : v); var = 0
      (7, 24),              # fewer pixels than row lanes, C < 64
      (31, 16),             # top of L = 1
      (32, 144),            # bottom of L = 2, a ragged 64-channel tile
      (75, 384),            # the shape of test_train_mobilenet.py
      (511, 96),            # top of L = 16
      (512, 576),           # L = 32, three blocks of the finish kernels with a ragged last
      (16750, 256)]         # P C / 4 = 1 072 000 > 4096 * 256: the apply kernels stride twice; leaf boundaries not divisible
# (P, Cin, Cout): wgrad, dgrad, dgrad + add
CONV1X1 = [(1, 4, 4), (40, 96, 96), (63, 16, 96), (65, 24, 144),
           (65, 144, 24),           # dgrad K = 24: a partial second K slice
           (70, 96, 4),             # a partial first K slice
           (130, 144, 24),          # wgrad L = 2, 65 pixels a leaf
           (1000, 32, 16),
           (4100, 16, 96),          # wgrad L = 32
           (1100, 576, 576),        # L = 8 because tiles * L < 512 binds; P alone would allow 16
           (128, 1028, 1028),       # L = 2, Cin Cout = 1 056 784 > 4096 * 256: the slab tree strides twice
           (8192, 576, 96)]         # block_13_expand at batch 8
# (B, H, W, C)
DW = [(1, 1, 1, 4), (1, 1, 7, 8), (1, 2, 1, 4), (2, 3, 5, 24), (1, 7, 4, 144), (3, 5, 5, 384),
      (1, 16, 33, 96),              # L = 32
      (2, 125, 67, 256)]            # 1 072 000 float4: the dgrad strides twice
# the INPUT's (B, H, W, C)
DW_S2 = [(1, 1, 1, 4), (1, 1, 2, 4), (1, 2, 2, 4), (1, 3, 2, 8), (1, 7, 12, 8), (2, 12, 7, 24), (1, 9, 9, 144), (2, 10, 10, 40),
         (1, 31, 64, 192),          # 16 x 32 outputs, L = 32
         (1, 250, 251, 96)]         # block_1-like, 1 506 000 float4: the dgrad strides twice, mixed parity
# (B, H, W, Cout)
STEM = [(1, 1, 1, 4), (1, 6, 5, 40), (1, 9, 13, 32),
        (1, 16, 15, 32),            # 64 outputs, L = 1
        (1, 32, 31, 8),             # L = 4
        (1, 128, 64, 32),           # L = 32: one full group of the two-level tree, seven absent
        (1, 128, 128, 32),          # L = 64
        (4, 92, 92, 32),            # L = 128
        (1, 256, 258, 12)]          # 16 512 outputs, L = 256: all eight groups
# margin per entry: MARGIN unless the CPU experiment above measures more for that entry (then ratio * 16 / 14.2, the same headroom)
MARGINS = {"conv1x1 dw": MARGIN, "conv1x1 dx": MARGIN, "conv1x1 dx+add": MARGIN, "dw dx": MARGIN, "dw dw": MARGIN, "dw_s2 dx": MARGIN,
           "dw_s2 dw": MARGIN, "stem dw": MARGIN}
GRID_ITEMS = 4096 * 256             # one pass of the grid-stride kernels


def a256(n):
    return (n + 255) & ~255


def out_side(n):
    return (n + n % 2 + 1 - 3) // 2 + 1


def pow2_leaves(total, slab, extra=0):
    """Every power of two L <= 256 with a256(L * slab) + extra == total."""
    return [n for n in (1 << k for k in range(9)) if a256(n * slab) + extra == total]


def bn_leaves(lib, P, C):
    """bytes = a256(L * 2 * C * 8) + a256(C * 4).  16 C bytes a leaf: from C = 16 on a256 grows strictly with L and the power of two
    is unique; below (C = 4: 1, 2 and 4 leaves all round to 256 bytes) the same P is asked again at C = 64 -- the header cuts `the
    pixels` into leaves -- and the answer must be one of the candidates."""
    found = pow2_leaves(lib.rpn_batchnorm_workspace_bytes(P, C), 2 * C * 8, a256(C * 4))
    if len(found) > 1:
        wide = pow2_leaves(lib.rpn_batchnorm_workspace_bytes(P, 64), 2 * 64 * 8, a256(64 * 4))
        assert len(wide) == 1 and wide[0] in found, (P, C, found, wide)
        return wide[0]
    assert len(found) == 1, (P, C, found)
    return found[0]


def conv1x1_leaves(lib, P, Cin, Cout):
    """bytes = L > 1 ? a256(L * Cin * Cout * 4) : 0.  Every shape of the table with a workspace has a slab above 256 bytes."""
    total = lib.rpn_conv1x1_wgrad_workspace_bytes(P, Cin, Cout)
    if total == 0:
        return 1
    found = [n for n in pow2_leaves(total, Cin * Cout * 4) if n > 1]
    assert len(found) == 1, (P, Cin, Cout, total, found)
    return found[0]


def unique_leaves(total, slab, shape):
    found = pow2_leaves(total, slab)                # slab >= 144 bytes > 128: a256(L * slab) grows strictly with L
    assert slab > 128 and len(found) == 1, (shape, total, found)
    return found[0]


def dw_leaves(lib, B, H, W, C):
    return unique_leaves(lib.rpn_dwconv3x3_wgrad_workspace_bytes(B, H, W, C), 9 * C * 4, (B, H, W, C))


def dw_s2_leaves(lib, B, H, W, C):
    return unique_leaves(lib.rpn_dwconv3x3_s2_wgrad_workspace_bytes(B, H, W, C), 9 * C * 4, (B, H, W, C))


def stem_leaves(lib, B, H, W, Cout):
    return unique_leaves(lib.rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(B, H, W, Cout), 27 * Cout * 4, (B, H, W, Cout))


# ---- float64 restatements of include/rpn_hip.h (dtype = float32 gives the yardsticks) -----------------------------------------------
def _bn(x, gamma, beta, dy, relu6, eps, mm0, mv0, dtype):
    x, gamma, beta, dy = (np.asarray(a, dtype) for a in (x, gamma, beta, dy))
    P = x.shape[0]
    n, eps = dtype(P), dtype(eps)
    mean = x.sum(0) / n
    var = ((x - mean) ** 2).sum(0) / n
    rstd = dtype(1) / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    pre = gamma * xhat + beta
    y = np.minimum(np.maximum(pre, dtype(0)), dtype(6)) if relu6 else pre
    dyp = np.where((pre > 0) & (pre < 6), dy, dtype(0)) if relu6 else dy          # TF's Relu6Grad: strict on both sides
    dbeta = dyp.sum(0)
    dgamma = (dyp * xhat).sum(0)
    dx = gamma * rstd * (dyp - dbeta / n - xhat * (dgamma / n))
    out = {"y": y, "mean": mean, "var": var, "dx": dx, "dgamma": dgamma, "dbeta": dbeta}
    if mm0 is not None:
        unbiased = var * n / (n - dtype(1)) if P > 1 else var                   # Bessel; one pixel has nothing to correct
        out["moving_mean"] = np.asarray(mm0, dtype) * dtype(MOM32) + mean * dtype(ONE_MINUS_MOM32)
        out["moving_var"] = np.asarray(mv0, dtype) * dtype(MOM32) + unbiased * dtype(ONE_MINUS_MOM32)
    assert all(v.dtype == dtype for v in out.values())
    return out, pre


def bn64(x, gamma, beta, dy, relu6, eps, mm0=None, mv0=None):
    """y, mean, var, dx, dgamma, dbeta (and the moving statistics after one step) of the header's BatchNorm; also the value before
    the ReLU6."""
    return _bn(x, gamma, beta, dy, relu6, eps, mm0, mv0, np.float64)


def bn32(x, gamma, beta, dy, relu6, eps):
    return _bn(x, gamma, beta, dy, relu6, eps, None, None, np.float32)[0]


def conv1x1_64(x, dy, w, add=None, dtype=np.float64):
    """dw (Cin, Cout) = x^T dy;  dx (P, Cin) = dy w^T (+ add)."""
    x, dy, w = (np.asarray(a, dtype) for a in (x, dy, w))
    dx = dy @ w.T
    if add is not None:
        dx = dx + np.asarray(add, dtype)
    dw = x.T @ dy
    assert dw.dtype == dtype and dx.dtype == dtype
    return dw, dx


def conv1x1_32(x, dy, w, add=None):
    return conv1x1_64(x, dy, w, add, np.float32)


def dw64(x, dy, w, dtype=np.float64):
    """stride 1 'same': dx[b][y][x][c] = sum_{r,s} dy[b][y+1-r][x+1-s][c] w[r][s][c];  dw[r][s][c] = sum_{b,y,x} x[b][y+r-1][x+s-1][c]
    dy[b][y][x][c]."""
    x, dy, w = (np.asarray(a, dtype) for a in (x, dy, w))
    B, H, W, C = dy.shape
    xp, dyp = np.zeros((B, H + 2, W + 2, C), dtype), np.zeros((B, H + 2, W + 2, C), dtype)
    xp[:, 1:H + 1, 1:W + 1], dyp[:, 1:H + 1, 1:W + 1] = x, dy
    dx, dw = np.zeros((B, H, W, C), dtype), np.zeros((3, 3, C), dtype)
    for r in range(3):
        for s in range(3):
            dx += dyp[:, 2 - r:2 - r + H, 2 - s:2 - s + W] * w[r, s]
            dw[r, s] = (xp[:, r:r + H, s:s + W] * dy).reshape(-1, C).sum(0)
    return dx, dw


def dw32(x, dy, w):
    return dw64(x, dy, w, np.float32)


def s2_tap(n, r):
    """One spatial dim of n input pixels under tap r: the outputs o whose input 2 o + r - n % 2 is inside, as (input slice, output
    slice); None when there are none."""
    p, on = n % 2, out_side(n)
    lo, hi = max(0, (p - r + 1) // 2), min(on - 1, (n - 1 + p - r) // 2)
    if hi < lo:
        return None
    return slice(2 * lo + r - p, 2 * hi + r - p + 1, 2), slice(lo, hi + 1)


def dw_s2_64(x, dy, w, dtype=np.float64):
    """stride 2 behind the padding before = n % 2, after = 1: dx[b][y][x][c] = sum_{r,s} dy[b][(y+pt-r)/2][(x+pl-s)/2][c] w[r][s][c]
    where both quotients are exact and in range;  dw[r][s][c] = sum_{b,oy,ox} x[b][2oy+r-pt][2ox+s-pl][c] dy[b][oy][ox][c]."""
    x, dy, w = (np.asarray(a, dtype) for a in (x, dy, w))
    B, H, W, C = x.shape
    assert dy.shape == (B, out_side(H), out_side(W), C)
    dx, dw = np.zeros((B, H, W, C), dtype), np.zeros((3, 3, C), dtype)
    for r in range(3):
        for s in range(3):
            ty, tx = s2_tap(H, r), s2_tap(W, s)
            if ty is None or tx is None:
                continue
            d = dy[:, ty[1], tx[1]]
            dx[:, ty[0], tx[0]] += d * w[r, s]
            dw[r, s] = (x[:, ty[0], tx[0]] * d).reshape(-1, C).sum(0)
    return dx, dw


def dw_s2_32(x, dy, w):
    return dw_s2_64(x, dy, w, np.float32)


def stem_wgrad64(x, dy, dtype=np.float64):
    """dw[r][s][ci][co] = sum_{b,oy,ox} x[b][2oy+r-pt][2ox+s-pl][ci] dy[b][oy][ox][co], x (B, H, W, 3)."""
    x, dy = np.asarray(x, dtype), np.asarray(dy, dtype)
    B, H, W, _ = x.shape
    Cout = dy.shape[3]
    assert dy.shape == (B, out_side(H), out_side(W), Cout)
    dw = np.zeros((3, 3, 3, Cout), dtype)
    for r in range(3):
        for s in range(3):
            ty, tx = s2_tap(H, r), s2_tap(W, s)
            if ty is not None and tx is not None:
                dw[r, s] = x[:, ty[0], tx[0]].reshape(-1, 3).T @ dy[:, ty[1], tx[1]].reshape(-1, Cout)
    assert dw.dtype == dtype
    return dw


def stem_wgrad32(x, dy):
    return stem_wgrad64(x, dy, np.float32)


# ---- the second float64 oracle: torch on the CPU --------------------------------------------------------------------------------------
def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def conv1x1_torch(x, dy, w):
    xt, wt = t64(x, True), t64(w, True)
    y = TF.conv2d(xt.t()[None, :, :, None], wt.t()[:, :, None, None])          # (1, Cout, P, 1)
    y.backward(t64(dy).t()[None, :, :, None])
    return wt.grad.numpy(), xt.grad.numpy()


def pad_s2(t):
    """Keras ZeroPadding2D(correct_pad(3)) on an NCHW tensor: F.pad(x, (pl, 1, pt, 1))."""
    return TF.pad(t, (t.shape[3] % 2, 1, t.shape[2] % 2, 1))


def dw_torch(x, dy, w, stride):
    xt, wt = t64(x, True), t64(w, True)
    k, nchw = wt.permute(2, 0, 1).unsqueeze(1), xt.permute(0, 3, 1, 2)
    y = TF.conv2d(nchw, k, padding=1, groups=x.shape[3]) if stride == 1 else TF.conv2d(pad_s2(nchw), k, stride=2, groups=x.shape[3])
    assert tuple(y.shape) == (dy.shape[0], dy.shape[3], dy.shape[1], dy.shape[2])
    y.backward(t64(dy).permute(0, 3, 1, 2))
    return xt.grad.numpy(), wt.grad.numpy()


def stem_torch(x, dy):
    wt = torch.zeros((3, 3, 3, dy.shape[3]), dtype=torch.float64, requires_grad=True)
    y = TF.conv2d(pad_s2(t64(x).permute(0, 3, 1, 2)), wt.permute(3, 2, 0, 1), stride=2)
    y.backward(t64(dy).permute(0, 3, 1, 2))
    return wt.grad.numpy()


# ---- data shaped like what the trainer feeds ------------------------------------------------------------------------------------------------
def relu6_like(rng, shape):
    """ReLU6 outputs in [0, 6]: about a third exactly 0 (37 %), some exactly 6 (5 %)."""
    return np.clip(1.0 + 3.0 * rng.standard_normal(shape), 0.0, 6.0).astype(np.float32)


def image_like(rng, shape):
    return rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)


def he1x1_like(rng, Cin, Cout):
    return (rng.standard_normal((Cin, Cout)) * math.sqrt(2.0 / Cin)).astype(np.float32)


def taps_like(rng, C):
    return (0.5 * rng.standard_normal((3, 3, C))).astype(np.float32)


def draw(build, base, alive):
    """The first of 32 seeds whose case has a gradient that is not all zero (half of dy is zero: one or two pixels can draw that)."""
    for seed in range(base, base + 32):
        case = build(np.random.RandomState(seed))
        if alive(case):
            return case
    raise AssertionError("no seed draws a non-zero gradient")


CLAMP_GAP, BN_ROUNDS = 1e-4, 8


def preact64(x, gamma, beta):
    x = x.astype(np.float64)
    mean = x.mean(0)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(0) + EPS32)
    return gamma * (x - mean) * rstd + beta, mean, rstd


def bn_case(P, C, relu6):
    """x (a conv output: signed; channel 5 with mean 100 and spread 0.1, channel 6 wide and off centre), gamma, beta, dy.  Every
    fourth channel has gamma about 3 and of every eight one has beta about -0.5 and one about 6.5, so that the ReLU6 clamps on both
    sides at every size.  With relu6, every float64 value before the clamp is kept CLAMP_GAP away from 0 and from 6: an element
    closer than twice that is moved to five times that distance on its own side, through x, and everything is recomputed (the move
    shifts the channel's mean and variance a little), for at most BN_ROUNDS rounds.  At P = 1 the value is beta whatever x is, and
    beta is drawn away from 0 and 6."""
    rng = np.random.RandomState(1000 * P + C)
    x = rng.standard_normal((P, C)).astype(np.float32)
    if C > 6:
        x[:, 5] = (100.0 + 0.1 * rng.standard_normal(P)).astype(np.float32)
        x[:, 6] = (-3.0 + 5.0 * rng.standard_normal(P)).astype(np.float32)
    gamma = rng.uniform(0.8, 1.2, C).astype(np.float32)
    gamma[0::4] = rng.uniform(2.5, 3.5, gamma[0::4].size)          # not channels 5 and 6: those stay as test_train_mobilenet.py has them
    beta = rng.uniform(2.7, 3.3, C).astype(np.float32)
    beta[2::8] = rng.uniform(-0.7, -0.3, beta[2::8].size)
    beta[3::8] = rng.uniform(6.3, 6.7, beta[3::8].size)
    dy = dy_like(rng, (P, C))
    if relu6:
        for _ in range(BN_ROUNDS + 1):
            pre, mean, rstd = preact64(x, gamma, beta)
            edge = np.where(np.abs(pre) <= np.abs(pre - 6.0), 0.0, 6.0)
            near = np.abs(pre - edge) < 2 * CLAMP_GAP
            if not near.any():
                break
            want = edge + np.where(pre >= edge, 5 * CLAMP_GAP, -5 * CLAMP_GAP)
            moved = mean + (want - beta) / (gamma.astype(np.float64) * rstd)
            x[near] = moved[near].astype(np.float32)
        gap = float(np.minimum(np.abs(pre), np.abs(pre - 6.0)).min())
        assert gap >= CLAMP_GAP, ("the builder leaves a value %.3g from the clamp" % gap, P, C)
    return x, gamma, beta, dy


# ---- CPU: the references judge each other before they judge a kernel ---------------------------------------------------------------------
def close13(a, b):
    assert a.shape == b.shape
    scale = np.abs(b).max()
    assert scale > 0 and np.abs(a - b).max() <= 1e-13 * scale, (a.shape, np.abs(a - b).max(), scale)


def test_canaries_are_nan_in_every_view():
    as32 = lambda word: struct.unpack("<f", struct.pack("<I", word))[0]
    as64 = lambda word: struct.unpack("<d", struct.pack("<II", word, word))[0]
    assert math.isnan(as32(CANARY)) and math.isnan(as32(CANARY64)) and math.isnan(as64(CANARY64))
    assert math.isfinite(as64(CANARY)) and 2.3e307 < as64(CANARY) < 2.4e307       # why the float64 workspace has its own canary
    assert CANARY64 < 2 ** 31                                                     # fits the int32 the bands are filled with


@pytest.mark.parametrize("relu6", [0, 1])
@pytest.mark.parametrize("P,C", [(2, 4), (3, 8), (7, 24), (32, 12), (75, 16)])
def test_references_agree_batchnorm(P, C, relu6):
    rng = np.random.RandomState(10 * P + C + relu6)
    x, dy = rng.standard_normal((P, C)).astype(np.float32), dy_like(rng, (P, C))
    gamma, beta = rng.uniform(0.8, 3.0, C).astype(np.float32), rng.uniform(0.0, 6.0, C).astype(np.float32)
    ref, pre = bn64(x, gamma, beta, dy, relu6, BN_EPS)
    tor, tpre = bn_torch(x, gamma, beta, dy, relu6, torch.float64)
    assert min(np.abs(pre).min(), np.abs(pre - 6.0).min()) > 1e-9                # no value on the clamp: the masks agree
    close13(pre, tpre)
    assert set(ref) == set(tor)
    for k in ref:
        close13(ref[k], tor[k])
    if relu6 and P * C >= 100:
        assert (pre <= 0).any() and (pre >= 6).any()
    f32 = bn32(x, gamma, beta, dy, relu6, BN_EPS)
    for k in ("mean", "var", "dbeta"):
        assert np.abs(f32[k] - ref[k]).max() <= 1e-5 * max(np.abs(ref[k]).max(), 1.0), k


def test_reference_batchnorm_over_one_pixel_is_the_closed_form():
    """torch refuses P = 1 in training mode: this case rests on the restatement alone, whose values are known."""
    with pytest.raises(ValueError):
        TF.batch_norm(torch.zeros((1, 4), dtype=torch.float64), None, None, training=True)
    x, dy = np.array([[1.5, -2.0, 0.25, 7.0]], np.float32), np.array([[1.0, -3.0, 0.5, 2.0]], np.float32)
    gamma, beta = np.array([1.0, 2.0, 3.0, 0.5], np.float32), np.array([3.0, -0.5, 6.5, 1.0], np.float32)
    mm0, mv0 = np.full(4, 0.5, np.float32), np.full(4, 2.0, np.float32)
    for relu6 in (0, 1):
        for ref in (bn64(x, gamma, beta, dy, relu6, BN_EPS, mm0, mv0)[0], bn32(x, gamma, beta, dy, relu6, BN_EPS)):
            assert np.array_equal(ref["mean"], x[0]) and not ref["var"].any() and not ref["dx"].any() and not ref["dgamma"].any()
            assert np.array_equal(ref["y"][0], np.clip(beta, 0, 6) if relu6 else beta)
            assert np.array_equal(ref["dbeta"], np.where((beta > 0) & (beta < 6), dy[0], 0) if relu6 else dy[0])
        ref = bn64(x, gamma, beta, dy, relu6, BN_EPS, mm0, mv0)[0]
        assert np.array_equal(ref["moving_var"], mv0.astype(np.float64) * MOM32) and np.isfinite(ref["moving_mean"]).all()


@pytest.mark.parametrize("P,Cin,Cout", [(1, 4, 4), (5, 4, 12), (17, 24, 8), (70, 12, 20)])
def test_references_agree_conv1x1(P, Cin, Cout):
    rng = np.random.RandomState(P + Cin + Cout)
    x, dy, w = relu6_like(rng, (P, Cin)), 1.0 + dy_like(rng, (P, Cout)), he1x1_like(rng, Cin, Cout)
    add = dy_like(rng, (P, Cin))
    dw, dx = conv1x1_64(x + 0.5, dy, w)
    tw, tx = conv1x1_torch(x + 0.5, dy, w)
    close13(dw, tw)
    close13(dx, tx)
    close13(conv1x1_64(x, dy, w, add)[1], tx + add.astype(np.float64))
    f_w, f_x = conv1x1_32(x + 0.5, dy, w, add)
    a_w, a_x = conv1x1_64(np.abs(x + 0.5), np.abs(dy), np.abs(w), np.abs(add))
    assert (np.abs(f_w - dw) <= P * U * a_w).all() and (np.abs(f_x - conv1x1_64(x, dy, w, add)[1]) <= (Cout + 1) * U * a_x).all()


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (1, 2, 1, 4), (2, 3, 5, 8), (1, 7, 4, 12), (3, 5, 5, 4)])
def test_references_agree_depthwise(B, H, W, C):
    rng = np.random.RandomState(B + 10 * H + 100 * W)
    x, dy, w = 0.5 + relu6_like(rng, (B, H, W, C)), 1.0 + dy_like(rng, (B, H, W, C)), taps_like(rng, C)
    dx, dw = dw64(x, dy, w)
    tx, tw = dw_torch(x, dy, w, 1)
    close13(dx, tx)
    close13(dw, tw)
    f_x, f_w = dw32(x, dy, w)
    a_x, a_w = dw64(np.abs(x), np.abs(dy), np.abs(w))
    assert (np.abs(f_x - dx) <= 9 * U * a_x).all() and (np.abs(f_w - dw) <= B * H * W * U * a_w).all()


S2_TINY = [(1, 1, 1, 4), (1, 1, 2, 4), (1, 2, 1, 4), (1, 2, 2, 4), (2, 3, 5, 8), (1, 7, 4, 12), (2, 6, 9, 4), (1, 8, 6, 8)]


@pytest.mark.parametrize("B,H,W,C", S2_TINY)
def test_references_agree_stride2(B, H, W, C):
    rng = np.random.RandomState(B + 10 * H + 100 * W)
    OH, OW = out_side(H), out_side(W)
    x, dy, w = 0.5 + relu6_like(rng, (B, H, W, C)), 1.0 + dy_like(rng, (B, OH, OW, C)), taps_like(rng, C)
    dx, dw = dw_s2_64(x, dy, w)
    tx, tw = dw_torch(x, dy, w, 2)
    close13(dx, tx)
    close13(dw, tw)
    f_x, f_w = dw_s2_32(x, dy, w)
    a_x, a_w = dw_s2_64(np.abs(x), np.abs(dy), np.abs(w))
    assert (np.abs(f_x - dx) <= 9 * U * a_x).all() and (np.abs(f_w - dw) <= B * OH * OW * U * a_w).all()
    img, g = image_like(rng, (B, H, W, 3)), 1.0 + dy_like(rng, (B, OH, OW, C))
    sw = stem_wgrad64(img, g)
    close13(sw, stem_torch(img, g))
    assert (np.abs(stem_wgrad32(img, g) - sw) <= B * OH * OW * U * stem_wgrad64(np.abs(img), np.abs(g))).all()


def test_stride2_agreement_shapes_have_every_parity():
    assert {(H % 2, W % 2) for _, H, W, _ in S2_TINY} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("P,C", BN)
def test_batchnorm_builder_keeps_every_value_off_the_clamp(P, C):
    """No case may be skipped because a value sits on the ReLU6 clamp: the builder must succeed for every shape of the table."""
    x, gamma, beta, dy = bn_case(P, C, 1)                                          # asserts the gap itself
    pre = preact64(x, gamma, beta)[0]
    assert min(np.abs(pre).min(), np.abs(pre - 6.0).min()) >= CLAMP_GAP
    assert (pre <= 0).any() and (pre >= 6).any() and ((pre > 0) & (pre < 6)).any()      # the mask is exercised on both sides
    if C > 6 and P >= 7:
        assert abs(x[:, 5].mean() - 100.0) < 0.5 and 0.03 < x[:, 5].std() < 0.3          # the channel E[x^2] - mean^2 gets wrong
    assert x.dtype == np.float32 and dy.dtype == np.float32 and (dy == 0).any()


def test_shape_tables_reach_every_path(lib):
    """Classifies the tables with the library's *_workspace_bytes functions, so that a later change of a leaf rule cannot silently
    empty a class."""
    bn = {s: bn_leaves(lib, *s) for s in BN}
    assert {1, 2, 16, 32} <= set(bn.values()), bn
    assert bn[(31, 16)] == 1 and bn[(32, 144)] == 2 and bn[(511, 96)] == 16 and bn[(512, 576)] == 32, bn     # both sides of two steps
    assert any(P < 16 for P, _ in BN) and any(P == 1 for P, _ in BN)
    assert any(C % 64 and C > 64 for _, C in BN) and any(C < 64 for _, C in BN) and any(C > 256 and C % 256 for _, C in BN)
    assert any(P * C // 4 > GRID_ITEMS and P % bn[(P, C)] for P, C in BN)

    cv = {s: conv1x1_leaves(lib, *s) for s in CONV1X1}
    assert {1, 2, 8, 32} <= set(cv.values()), cv
    capped = [(P, Cin, Cout) for (P, Cin, Cout), n in cv.items()
              if ((Cin + 63) // 64) * ((Cout + 63) // 64) * n >= 512 and P // (2 * n) >= 64 and n < 32]
    assert any(cv[s] == 8 and s[0] // 16 >= 64 > s[0] // 32 for s in capped), (cv, capped)      # 8 by the cap; P alone allows 16
    assert any(n == 2 and (P // 2) % 2 for (P, _, _), n in cv.items())                            # two leaves of an odd length
    assert {Cout % 16 for _, _, Cout in CONV1X1} >= {0, 4, 8}
    assert any(Cout < 16 for _, _, Cout in CONV1X1) and any(16 < Cout < 32 for _, _, Cout in CONV1X1)
    assert any(P % 64 for P, _, _ in CONV1X1) and any(P < 64 for P, _, _ in CONV1X1) and any(Cin % 64 for _, Cin, _ in CONV1X1)
    assert any(Cin * Cout > GRID_ITEMS and cv[(P, Cin, Cout)] > 1 for P, Cin, Cout in CONV1X1)
    assert (8192, 576, 96) in cv

    dw = {s: dw_leaves(lib, *s) for s in DW}
    assert {1, 32} <= set(dw.values()), dw
    assert any(B * H * W * C // 4 > GRID_ITEMS for B, H, W, C in DW) and any(H != W for _, H, W, _ in DW)
    assert any(C < 64 for *_, C in DW) and any(C % 64 and C > 64 for *_, C in DW) and any(H == 1 for _, H, _, _ in DW)

    s2 = {s: dw_s2_leaves(lib, *s) for s in DW_S2}
    assert {1, 32} <= set(s2.values()), s2
    assert {(H % 2, W % 2) for _, H, W, _ in DW_S2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(C < 32 for *_, C in DW_S2) and any(C % 32 and C > 32 for *_, C in DW_S2)
    assert any(B * H * W * C // 4 > GRID_ITEMS and H % 2 != W % 2 for B, H, W, C in DW_S2)

    st = {s: stem_leaves(lib, *s) for s in STEM}
    assert {1, 32, 64, 128, 256} <= set(st.values()), st
    assert any(Cout % 32 and Cout > 32 for *_, Cout in STEM) and any(Cout < 32 for *_, Cout in STEM)
    assert st[(1, 16, 15, 32)] == 1 and out_side(16) * out_side(15) == 64


# ---- GPU: every call inside guard bands, twice, the inputs untouched ----------------------------------------------------------------------
def call(what, fn, inputs, outputs, need=0, ws_canary=CANARY, runs=2):
    """fn(bands, ws_ptr, need) -> status.  inputs: name -> array.  outputs: name -> shape, or an array the call updates in place (a
    fresh band with that data in every run).  Returns the outputs of the first run, after same_bytes over all runs."""
    bands = {k: Band(v.size, v) for k, v in inputs.items()}
    before = {k: bands[k].buf.clone() for k in inputs}
    got = []
    for _ in range(runs):
        if need:
            assert need % 16 == 0
            bands["ws"] = workspace(need) if ws_canary == CANARY else Band(need // 4, canary=ws_canary)
        for k, v in outputs.items():
            bands[k] = Band(v.size, v) if isinstance(v, np.ndarray) else Band(int(np.prod(v)))
        L.check(fn(bands, bands["ws"].ptr if need else None, need), what)
        settle(bands, tuple(outputs))
        got.append(tuple(bands[k].numpy(v.shape if isinstance(v, np.ndarray) else v) for k, v in outputs.items()))
    for k in inputs:
        assert torch.equal(bands[k].buf, before[k]), "%s changed input %s" % (what, k)
    return same_bytes(got)


def gpu_bn_forward(lib, x, gamma, beta, relu6, mm0=None, mv0=None):
    P, C = x.shape
    outputs = {"y": (P, C), "mean": (C,), "var": (C,)}
    if mm0 is not None:
        outputs.update(mm=mm0, mv=mv0)
    return call("rpn_batchnorm_train_forward", lambda b, ws, need: lib.rpn_batchnorm_train_forward(
        b["x"].ptr, P, C, b["gamma"].ptr, b["beta"].ptr, relu6, BN_EPS, BN_MOMENTUM, b["y"].ptr, b["mean"].ptr, b["var"].ptr,
        b["mm"].ptr if mm0 is not None else None, b["mv"].ptr if mm0 is not None else None, ws, need, L.stream_ptr()),
        {"x": x, "gamma": gamma, "beta": beta}, outputs, lib.rpn_batchnorm_workspace_bytes(P, C), CANARY64)


def gpu_bn_backward(lib, x, dy, gamma, beta, mean, var, relu6, in_place=False):
    P, C = x.shape
    inputs = {"x": x, "gamma": gamma, "beta": beta, "mean": mean, "var": var}
    outputs = {"dx": dy if in_place else (P, C), "dgamma": (C,), "dbeta": (C,)}           # in place: d_dx == d_dy, as documented
    if not in_place:
        inputs["dy"] = dy
    return call("rpn_batchnorm_train_backward", lambda b, ws, need: lib.rpn_batchnorm_train_backward(
        b["x"].ptr, b["dx" if in_place else "dy"].ptr, P, C, b["gamma"].ptr, b["beta"].ptr, b["mean"].ptr, b["var"].ptr, relu6, BN_EPS,
        b["dx"].ptr, b["dgamma"].ptr, b["dbeta"].ptr, ws, need, L.stream_ptr()),
        inputs, outputs, lib.rpn_batchnorm_workspace_bytes(P, C), CANARY64)


def gpu_conv1x1_wgrad(lib, x, dy):
    (P, Cin), Cout = x.shape, dy.shape[1]
    return call("rpn_conv1x1_wgrad", lambda b, ws, need: lib.rpn_conv1x1_wgrad(b["x"].ptr, b["dy"].ptr, P, Cin, Cout, b["dw"].ptr, ws, need,
                                                                               L.stream_ptr()),
                {"x": x, "dy": dy}, {"dw": (Cin, Cout)}, lib.rpn_conv1x1_wgrad_workspace_bytes(P, Cin, Cout))[0]


def gpu_conv1x1_dgrad(lib, dy, w, add=None):
    (P, Cout), Cin = dy.shape, w.shape[0]
    inputs = {"dy": dy, "w": w}
    if add is not None:
        inputs["add"] = add
    return call("rpn_conv1x1_dgrad", lambda b, ws, need: lib.rpn_conv1x1_dgrad(b["dy"].ptr, b["w"].ptr, b["add"].ptr if add is not None else None,
                                                                               P, Cin, Cout, b["dx"].ptr, L.stream_ptr()),
                inputs, {"dx": (P, Cin)})[0]


def gpu_depthwise(lib, stride, x, dy, w):
    """dx and dw of the depthwise pair at the given stride."""
    B, H, W, C = x.shape
    dgrad, wgrad, size_fn = (lib.rpn_dwconv3x3_dgrad, lib.rpn_dwconv3x3_wgrad, lib.rpn_dwconv3x3_wgrad_workspace_bytes) if stride == 1 else \
        (lib.rpn_dwconv3x3_s2_dgrad, lib.rpn_dwconv3x3_s2_wgrad, lib.rpn_dwconv3x3_s2_wgrad_workspace_bytes)
    name = "rpn_dwconv3x3%s_" % ("" if stride == 1 else "_s2")
    dx = call(name + "dgrad", lambda b, ws, need: dgrad(b["dy"].ptr, b["w"].ptr, B, H, W, C, b["dx"].ptr, L.stream_ptr()),
              {"dy": dy, "w": w}, {"dx": (B, H, W, C)})[0]
    dw = call(name + "wgrad", lambda b, ws, need: wgrad(b["x"].ptr, b["dy"].ptr, B, H, W, C, b["dw"].ptr, ws, need, L.stream_ptr()),
              {"x": x, "dy": dy}, {"dw": (3, 3, C)}, size_fn(B, H, W, C))[0]
    return dx, dw


def gpu_stem_wgrad(lib, x, dy):
    (B, H, W, _), Cout = x.shape, dy.shape[3]
    return call("rpn_conv3x3_s2_cin3_wgrad", lambda b, ws, need: lib.rpn_conv3x3_s2_cin3_wgrad(b["x"].ptr, b["dy"].ptr, B, H, W, Cout,
                                                                                               b["dw"].ptr, ws, need, L.stream_ptr()),
                {"x": x, "dy": dy}, {"dw": (3, 3, 3, Cout)}, lib.rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(B, H, W, Cout))[0]


# ---- GPU: integers, bit for bit over the whole tables (every element compared) -----------------------------------------------------------
# |values| <= 3: every partial sum stays below 9 * 16 512 (the longest sum of the tables) < 2^24 -- exact in float32 whatever the order
def exact(got, ref64):
    assert got.dtype == np.float32 and np.array_equal(got, ref64.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("P,Cin,Cout", CONV1X1)
def test_conv1x1_integers_bit_exact_inside_guard_bands(lib, P, Cin, Cout):
    rng = np.random.RandomState(P + Cin + Cout)
    x, dy, w, add = ints(rng, (P, Cin)), ints(rng, (P, Cout)), ints(rng, (Cin, Cout)), ints(rng, (P, Cin))
    dw, dx = conv1x1_64(x, dy, w)
    exact(gpu_conv1x1_wgrad(lib, x, dy), dw)
    exact(gpu_conv1x1_dgrad(lib, dy, w), dx)
    exact(gpu_conv1x1_dgrad(lib, dy, w, add), dx + add)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C", DW)
def test_depthwise_integers_bit_exact_inside_guard_bands(lib, B, H, W, C):
    rng = np.random.RandomState(B * H + W + C)
    x, dy, w = ints(rng, (B, H, W, C)), ints(rng, (B, H, W, C)), ints(rng, (3, 3, C))
    dx, dw = gpu_depthwise(lib, 1, x, dy, w)
    ref_x, ref_w = dw64(x, dy, w)
    exact(dx, ref_x)
    exact(dw, ref_w)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C", DW_S2)
def test_depthwise_stride2_integers_bit_exact_inside_guard_bands(lib, B, H, W, C):
    rng = np.random.RandomState(B * H + W + C)
    x, dy, w = ints(rng, (B, H, W, C)), ints(rng, (B, out_side(H), out_side(W), C)), ints(rng, (3, 3, C))
    dx, dw = gpu_depthwise(lib, 2, x, dy, w)
    ref_x, ref_w = dw_s2_64(x, dy, w)
    exact(dx, ref_x)
    exact(dw, ref_w)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cout", STEM)
def test_stem_wgrad_integers_bit_exact_inside_guard_bands(lib, B, H, W, Cout):
    rng = np.random.RandomState(B * H + W + Cout)
    x, dy = ints(rng, (B, H, W, 3)), ints(rng, (B, out_side(H), out_side(W), Cout))
    exact(gpu_stem_wgrad(lib, x, dy), stem_wgrad64(x, dy))


@pytest.mark.gpu
@pytest.mark.parametrize("relu6", [0, 1])
@pytest.mark.parametrize("P,C", BN)
def test_batchnorm_exact_cases_inside_guard_bands(lib, P, C, relu6):
    """The cases BatchNorm has exact answers for.  Even channels: x constant (a multiple of 1/4 up to 4: every sum and sum of squares
    is exact in float64) -- mean exactly the constant, var exactly 0, xhat exactly 0, so y = clamp(beta), dgamma = 0 and dbeta = sum
    dy [0 < beta < 6], with beta drawn from {-1, 0, 3, 6, 7}: the mask is strict on both sides.  Odd channels, when P is even: x in
    {a, -a} in equal numbers, a a power of two -- mean exactly 0, var exactly a^2; there gamma = 1 and beta = 3 keep y near 2 and 4,
    inside the clamp, so dbeta = sum dy (integers: exact)."""
    rng = np.random.RandomState(P + C + relu6)
    x = np.zeros((P, C), np.float32)
    const = (rng.randint(-16, 17, size=C) / 4.0).astype(np.float32)
    x[:] = const
    a = (2.0 ** rng.randint(-3, 4, size=C)).astype(np.float32)
    gamma, beta = ints(rng, (C,), 1, 4), rng.choice(np.array([-1.0, 0.0, 3.0, 6.0, 7.0], np.float32), size=C)
    two = np.zeros(C, bool)
    if P % 2 == 0:
        two[1::2] = True
        signs = np.where(rng.permutation(P) < P // 2, 1.0, -1.0).astype(np.float32)
        x[:, two] = signs[:, None] * a[two]
        gamma[two], beta[two] = 1.0, 3.0
    dy = ints(rng, (P, C))
    mm0, mv0 = rng.uniform(-0.1, 0.1, C).astype(np.float32), rng.uniform(0.8, 1.2, C).astype(np.float32)
    y, mean, var, mm, mv = gpu_bn_forward(lib, x, gamma, beta, relu6, mm0, mv0)
    exact(mean, np.where(two, 0.0, const))
    exact(var, np.where(two, a.astype(np.float64) ** 2, 0.0))
    want_y = np.broadcast_to(np.clip(beta, 0.0, 6.0) if relu6 else beta, (P, C))
    assert np.array_equal(y[:, ~two], want_y[:, ~two])
    ref = bn64(x, gamma, beta, dy, relu6, EPS32, mm0, mv0)[0]
    assert np.array_equal(ref["mean"], np.where(two, 0.0, const)) and np.array_equal(ref["var"], np.where(two, a.astype(np.float64) ** 2, 0.0))
    assert np.allclose(y, ref["y"], rtol=1e-6, atol=0)
    assert np.allclose(mm, ref["moving_mean"], rtol=5e-7, atol=1e-9) and np.allclose(mv, ref["moving_var"], rtol=5e-7, atol=0)
    dx, dgamma, dbeta = gpu_bn_backward(lib, x, dy, gamma, beta, mean, var, relu6)
    exact(dbeta, ref["dbeta"])
    live = (beta > 0) & (beta < 6) if relu6 else np.ones(C, bool)
    assert np.array_equal(dbeta, np.where(live, dy.astype(np.float64).sum(0), 0.0).astype(np.float32))
    assert not dgamma[~two].any()
    # |xhat| < 1 in the two-valued channels; where the signed sum of dy cancels, float64 itself leaves 1e-15, not 0
    assert (np.abs(dgamma - ref["dgamma"]) <= 1e-6 * np.abs(dy).sum(0)).all()
    assert np.abs(dx - ref["dx"]).max() <= 1e-5 * max(np.abs(ref["dx"]).max(), 1.0)


# ---- GPU: real values against float64 ---------------------------------------------------------------------------------------------------------
def parity(what, shape, got, ref, f32, absprod, n, depth):
    """err(gpu) <= MARGINS[what] * max(e32, 2^-24) and |got - ref| <= (n + depth) 2^-24 (|A| . |B|) element-wise; prints the errors."""
    scale = np.abs(ref).max()
    assert scale > 0 and got.shape == ref.shape == f32.shape and f32.dtype == np.float32, (what, shape)
    d = np.abs(got - ref)
    e_gpu, e32 = d.max() / scale, np.abs(f32 - ref).max() / scale
    print("parity %-14s %-24s err_gpu %.2e  e32 %.2e  err/bound %.3f" % (what, shape, e_gpu, e32, e_gpu / (MARGINS[what] * max(e32, U))))
    assert e_gpu <= MARGINS[what] * max(e32, U), (what, shape, e_gpu, e32)
    assert (d <= (n + depth) * U * absprod).all(), (what, shape, "beyond the rigorous float32 bound")


@pytest.mark.gpu
@pytest.mark.parametrize("P,Cin,Cout", CONV1X1)
def test_conv1x1_real_values_match_float64(lib, P, Cin, Cout):
    x, dy, w, add = draw(lambda rng: (relu6_like(rng, (P, Cin)), dy_like(rng, (P, Cout)), he1x1_like(rng, Cin, Cout), dy_like(rng, (P, Cin))),
                         4000 + P + Cin + Cout, lambda c: (c[0].T @ c[1]).any() and c[1].any() and c[3].any())
    shape = (P, Cin, Cout)
    (r_w, r_x), (f_w, f_x) = conv1x1_64(x, dy, w), conv1x1_32(x, dy, w)
    a_w, a_x = conv1x1_64(np.abs(x), np.abs(dy), np.abs(w))
    depth = int(math.log2(conv1x1_leaves(lib, P, Cin, Cout)))
    parity("conv1x1 dw", shape, gpu_conv1x1_wgrad(lib, x, dy), r_w, f_w, a_w, P, depth)
    parity("conv1x1 dx", shape, gpu_conv1x1_dgrad(lib, dy, w), r_x, f_x, a_x, Cout, 0)
    parity("conv1x1 dx+add", shape, gpu_conv1x1_dgrad(lib, dy, w, add), conv1x1_64(x, dy, w, add)[1], conv1x1_32(x, dy, w, add)[1],
           a_x + np.abs(add), Cout, 1)


def depthwise_parity(lib, stride, shape, leaves, lanes):
    B, H, W, C = shape
    oshape = shape if stride == 1 else (B, out_side(H), out_side(W), C)
    ref_fn, f32_fn = (dw64, dw32) if stride == 1 else (dw_s2_64, dw_s2_32)
    x, dy, w = draw(lambda rng: (relu6_like(rng, shape), dy_like(rng, oshape), taps_like(rng, C)), 5000 + B + H + W + C,
                    lambda c: ref_fn(c[0], c[1], c[2])[1].any())
    (r_x, r_w), (f_x, f_w), (a_x, a_w) = ref_fn(x, dy, w), f32_fn(x, dy, w), ref_fn(x, np.abs(dy), np.abs(w))     # x >= 0 already
    dx, dw = gpu_depthwise(lib, stride, x, dy, w)
    name = "dw" if stride == 1 else "dw_s2"
    parity(name + " dx", shape, dx, r_x, f_x, a_x, 9, 0)
    # a lane's chain, the lanes of a leaf in order, the leaves in a tree
    parity(name + " dw", shape, dw, r_w, f_w, a_w, oshape[0] * oshape[1] * oshape[2], lanes + int(math.log2(leaves)))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C", DW)
def test_depthwise_real_values_match_float64(lib, B, H, W, C):
    depthwise_parity(lib, 1, (B, H, W, C), dw_leaves(lib, B, H, W, C), 16)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C", DW_S2)
def test_depthwise_stride2_real_values_match_float64(lib, B, H, W, C):
    depthwise_parity(lib, 2, (B, H, W, C), dw_s2_leaves(lib, B, H, W, C), 32)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cout", STEM)
def test_stem_wgrad_real_values_match_float64(lib, B, H, W, Cout):
    oshape = (B, out_side(H), out_side(W), Cout)
    x, dy = draw(lambda rng: (image_like(rng, (B, H, W, 3)), dy_like(rng, oshape)), 6000 + B + H + W + Cout,
                 lambda c: stem_wgrad64(c[0], c[1]).any())
    leaves = stem_leaves(lib, B, H, W, Cout)
    parity("stem dw", (B, H, W, Cout), gpu_stem_wgrad(lib, x, dy), stem_wgrad64(x, dy), stem_wgrad32(x, dy),
           stem_wgrad64(np.abs(x), np.abs(dy)), B * oshape[1] * oshape[2], 32 + int(math.log2(leaves)))


def rel_dev(a, ref):
    """max |a - ref| / max |ref|; where the reference is all zero (var, dx and dgamma over one pixel) only zeros deviate by 0."""
    scale = np.abs(ref).max()
    d = np.abs(np.asarray(a, np.float64) - ref).max()
    return float(d / scale) if scale > 0 else (0.0 if d == 0 else math.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("relu6", [0, 1])
@pytest.mark.parametrize("P,C", BN)
def test_batchnorm_real_values_match_float64(lib, P, C, relu6):
    """The bound of test_train_mobilenet.py: 4 x the largest deviation of torch float32 from torch float64 over the six outputs, each
    relative to max |reference| of that output; at P = 1, where torch cannot serve, of the numpy float32 yardstick (there every
    output is exact in every arithmetic: the bound is 0 and holds)."""
    x, gamma, beta, dy = bn_case(P, C, relu6)
    mm0 = np.random.RandomState(P).uniform(-0.1, 0.1, C).astype(np.float32)
    mv0 = np.random.RandomState(C).uniform(0.8, 1.2, C).astype(np.float32)
    ref, pre = bn64(x, gamma, beta, dy, relu6, EPS32, mm0, mv0)
    keys = ("y", "mean", "var", "dx", "dgamma", "dbeta")
    if P > 1:
        t32 = bn_torch(x, gamma, beta, dy, relu6, torch.float32)[0]
    else:
        t32 = bn32(x, gamma, beta, dy, relu6, EPS32)
    bound = 4.0 * max(rel_dev(t32[k], ref[k]) for k in keys)
    if relu6:
        assert (pre <= 0).any() and (pre >= 6).any()
    y, mean, var, mm, mv = gpu_bn_forward(lib, x, gamma, beta, relu6, mm0, mv0)
    dx, dgamma, dbeta = gpu_bn_backward(lib, x, dy, gamma, beta, mean, var, relu6)
    got = {"y": y, "mean": mean, "var": var, "dx": dx, "dgamma": dgamma, "dbeta": dbeta}
    devs = {k: rel_dev(got[k], ref[k]) for k in keys}
    print("batchnorm (%d, %d) relu6=%d: bound %.3g  worst %.3g  err/bound %.3f  %s"
          % (P, C, relu6, bound, max(devs.values()), max(devs.values()) / bound if bound else 0.0, {k: "%.3g" % v for k, v in devs.items()}))
    for k, v in devs.items():
        assert v <= bound, (k, v, bound)
    if C > 6 and P >= 7:
        assert rel_dev(var[5:6], ref["var"][5:6]) < 1e-3                        # the channel the naive formula gets wrong
    assert np.allclose(mm, ref["moving_mean"], rtol=5e-7, atol=1e-9) and np.allclose(mv, ref["moving_var"], rtol=5e-7, atol=0)
    # both moving pointers NULL: the same y, mean and var
    same_bytes([(y, mean, var), gpu_bn_forward(lib, x, gamma, beta, relu6)])
    # d_dx == d_dy: the same bytes as out of place
    same_bytes([(dx, dgamma, dbeta), gpu_bn_backward(lib, x, dy, gamma, beta, mean, var, relu6, in_place=True)])


@pytest.mark.gpu
@pytest.mark.parametrize("P,C", [(512, 576), (16750, 256)])
def test_batchnorm_backward_mask_is_the_forward_clamp(lib, P, C):
    """The backward recomputes y; this ties that recomputation to the forward's own output without a tolerance.  dy = 1 exactly where
    the forward's y is 0 or 6 and 0 elsewhere: dbeta, dgamma and dx all zero.  dy = 1 exactly where 0 < y < 6: dbeta[c] is that
    count (at most 16 750 ones: exact)."""
    x, gamma, beta, _ = bn_case(P, C, 1)
    y, mean, var = gpu_bn_forward(lib, x, gamma, beta, 1)
    clamped = (y == 0) | (y == 6)
    assert clamped.any() and (y == 0).any() and (y == 6).any() and not clamped.all()
    dx, dgamma, dbeta = gpu_bn_backward(lib, x, clamped.astype(np.float32), gamma, beta, mean, var, 1)
    assert not dbeta.any() and not dgamma.any() and not dx.any()
    dx, dgamma, dbeta = gpu_bn_backward(lib, x, (~clamped).astype(np.float32), gamma, beta, mean, var, 1)
    assert np.array_equal(dbeta, (~clamped).sum(0).astype(np.float32))
