"""CPU suite, RoI max pooling: the numpy restatement of the contract (the oracle of tests/test_gpu_roi_max.py), its known answers,
the C ABI boundary without a device, the code-object figures of the new kernels and DetectionHead.load_keras_weights' checks.

The contract (include/rpn_hip.h), float32, every operation rounded on its own, per axis (y shown):
    a = y1 * Sy;  e = y2 * Sy;  a NaN product (of the four) -> the RoI is dead;  both clamped to [-2^20, 2^20]
    p1 = (int)roundf(a);  p2 = (int)roundf(e)  (half away from zero);  n = max(p2 - p1 + 1, 1);  bin = (float)n / (float)ph
    bin i covers rows [hs, he):  hs = min(max((int)floorf((float)i * bin) + p1, 0), H)
                                 he = min(max((int)ceilf((float)(i + 1) * bin) + p1, 0), H)
    empty bin (he <= hs or we <= ws): +0.0 and argmax -1.  Otherwise scan in (row, column) order from the first pixel; a later
    pixel v replaces (m, idx) iff v > m || v != v.  Rows r >= valid[b] and dead RoIs: +0.0 and -1.
    default extent (H - 1, W - 1); an axis of one pixel takes 1 (the extent must be > 0).
Backward: dx[b, y, x, c] = the float32 sum, in (r, i, j) order from +0.0, of the dy[b, r, i, j, c] with argmax == y * W + x.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from test_roi_host import BOX_KINDS, interior_boxes, nasty_boxes
from tf_rpn_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rpn_roi_max_pool", "rpn_roi_max_pool_backward", "rpn_model_roi_max_pool")
F = np.float32
CLAMP = F(2.0 ** 20)
U = 2.0 ** -24


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _roundf(a):
    """C's roundf on a finite float32: to nearest, halves away from zero (a - trunc(a) is exact)"""
    t = np.trunc(a)
    return int(t) + (int(np.sign(a)) if abs(F(a - t)) >= F(0.5) else 0)


def default_extent(H, W):
    return (max(H - 1, 1), max(W - 1, 1))


def _axis(c1, c2, extent, n, size):
    """-> (lo, hi): (n,) int64 pixel limits [lo, hi) of the n bins, or None when a product is NaN (the RoI is dead)"""
    with np.errstate(invalid="ignore", over="ignore"):
        a, e = F(F(c1) * F(extent)), F(F(c2) * F(extent))
    if np.isnan(a) or np.isnan(e):
        return None
    a, e = min(max(a, -CLAMP), CLAMP), min(max(e, -CLAMP), CLAMP)
    p1, p2 = _roundf(a), _roundf(e)
    bin_ = F(F(max(p2 - p1 + 1, 1)) / F(n))
    i = np.arange(n, dtype=np.float32)
    lo = np.floor((i * bin_).astype(np.float32)).astype(np.int64) + p1
    hi = np.ceil(((i + F(1)) * bin_).astype(np.float32)).astype(np.int64) + p1
    return np.clip(lo, 0, size), np.clip(hi, 0, size)


def _live(valid, b, R):
    return R if valid is None else min(max(int(valid[b]), 0), R)


def roi_max_pool_ref(x, rois, ph, pw, extent=None, valid=None, fast=False):
    """x (B,H,W,C) float32, rois (B,R,4) [y1,x1,y2,x2] normalised -> (out (B,R,ph,pw,C) float32, argmax (B,R,ph,pw,C) int32).
    The scan is the contract's, pixel by pixel.  ``fast`` (for the large cases of the GPU suite): a bin without a NaN takes
    numpy's argmax over its pixels in scan order instead -- the first maximum, +0 and -0 comparing equal: what the scan gives
    (test_fast_restatement_is_the_scan holds the two together); a bin with a NaN is still scanned."""
    x, rois = np.ascontiguousarray(x, dtype=np.float32), np.asarray(rois, dtype=np.float32)
    B, H, W, C = x.shape
    R = rois.shape[1]
    sy, sx = default_extent(H, W) if extent is None else extent
    out = np.zeros((B, R, ph, pw, C), dtype=np.float32)
    argmax = np.full((B, R, ph, pw, C), -1, dtype=np.int32)
    for b in range(B):
        for r in range(_live(valid, b, R)):
            y1, x1, y2, x2 = rois[b, r]
            ay, ax = _axis(y1, y2, sy, ph, H), _axis(x1, x2, sx, pw, W)
            if ay is None or ax is None:
                continue
            for i in range(ph):
                hs, he = int(ay[0][i]), int(ay[1][i])
                for j in range(pw):
                    ws, we = int(ax[0][j]), int(ax[1][j])
                    if he <= hs or we <= ws:
                        continue
                    if fast:
                        block = x[b, hs:he, ws:we].reshape(-1, C)
                        if not np.isnan(block).any():
                            k = block.argmax(axis=0)
                            out[b, r, i, j] = block[k, np.arange(C)]
                            argmax[b, r, i, j] = (hs + k // (we - ws)) * W + ws + k % (we - ws)
                            continue
                    m = x[b, hs, ws].copy()
                    idx = np.full((C,), hs * W + ws, dtype=np.int32)
                    for y in range(hs, he):
                        for xx in range(ws, we):
                            v = x[b, y, xx]
                            with np.errstate(invalid="ignore"):
                                take = (v > m) | (v != v)
                            m = np.where(take, v, m)
                            idx = np.where(take, np.int32(y * W + xx), idx)
                    out[b, r, i, j], argmax[b, r, i, j] = m, idx
    return out, argmax


def roi_max_pool_backward_ref(dy, argmax, shape, valid=None):
    """-> (dx float32 summed in float32 in (r, i, j) order, dx float64, n = the number of terms of every element, S = the sum of
    their |dy|): the bound of the float32 sum against the float64 one is (n - 1) u S, u = 2^-24 (a sequential sum of n terms)."""
    dy, argmax = np.asarray(dy, dtype=np.float32), np.asarray(argmax)
    B, H, W, C = shape
    R, ph, pw = dy.shape[1:4]
    dx = np.zeros((B, H * W, C), dtype=np.float32)
    dx64, S = np.zeros((B, H * W, C)), np.zeros((B, H * W, C))
    n = np.zeros((B, H * W, C), dtype=np.int64)
    cs = np.arange(C)
    for b in range(B):
        for r in range(_live(valid, b, R)):
            for i in range(ph):
                for j in range(pw):
                    idx, g = argmax[b, r, i, j], dy[b, r, i, j]
                    k = idx >= 0
                    if not k.any():
                        continue
                    at = (b, idx[k], cs[k])                 # (one term per channel: no index repeats)
                    dx[at] = dx[at] + g[k]                  # float32 + float32, rounded once
                    dx64[at] += g[k].astype(np.float64)
                    S[at] += np.abs(g[k]).astype(np.float64)
                    n[at] += 1
    return tuple(a.reshape(B, H, W, C) for a in (dx, dx64, n, S))


def backward_bound(n, S):
    """the issue's bound on |dx32 - dx64| per element"""
    return 1.01 * np.maximum(n - 1, 0) * U * S


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_roundf_is_half_away_from_zero():
    for a, want in ((0.5, 1), (-0.5, -1), (1.5, 2), (2.5, 3), (-2.5, -3), (0.49999997, 0), (-0.49999997, 0), (30.0, 30), (1048576.0, 1048576)):
        assert _roundf(F(a)) == want, a


@pytest.mark.parametrize("n", [1, 2, 7, 31])
def test_identity_known_answer(n):
    """Box [0,0,1,1], ph = pw = H = W, default extent: p1 = 0, p2 = H - 1, bin = 1, every bin is one pixel."""
    x = np.random.RandomState(n).standard_normal((1, n, n, 4)).astype(np.float32)
    out, argmax = roi_max_pool_ref(x, np.array([[[0, 0, 1, 1]]], np.float32), n, n)
    assert np.array_equal(out[0, 0].view(np.uint32), x[0].view(np.uint32))
    assert np.array_equal(argmax[0, 0], np.broadcast_to(np.arange(n * n).reshape(n, n, 1), (n, n, 4)))


def test_constant_map_takes_each_bins_first_pixel_and_negative_map_stays_negative():
    rng = np.random.RandomState(1)
    rois = interior_boxes(rng, 1, 6)
    H, W = 9, 11
    out, argmax = roi_max_pool_ref(np.full((1, H, W, 4), 2.5, np.float32), rois, 3, 4)
    assert (out == 2.5).all()
    for r in range(6):
        (ylo, _), (xlo, _) = _axis(rois[0, r, 0], rois[0, r, 2], H - 1, 3, H), _axis(rois[0, r, 1], rois[0, r, 3], W - 1, 4, W)
        assert np.array_equal(argmax[0, r, :, :, 0], ylo[:, None] * W + xlo[None, :])
    out, _ = roi_max_pool_ref(np.full((1, H, W, 4), -1.0, np.float32), rois, 3, 4)
    assert (out == -1.0).all()                                                     # not 0
    out, _ = roi_max_pool_ref(np.full((1, H, W, 4), -np.inf, np.float32), rois, 3, 4)
    assert np.isneginf(out).all()
    x = np.zeros((1, H, W, 4), np.float32)
    x[0, :, :, 1] = -0.0                                                           # the sign of zero is copied
    out, _ = roi_max_pool_ref(x, rois, 3, 4)
    assert not np.signbit(out[..., 0]).any() and np.signbit(out[..., 1]).all()


def test_bins_narrower_than_a_pixel_share_pixels_and_the_backward_sums_them():
    """ph = pw = 7 on a 2 x 2 map: n = 2 < 7, every pixel lies in several bins; dx of a pixel is the sum of dy over the bins that
    chose it, and the sum over dx is the sum of dy over the live non-empty bins."""
    rng = np.random.RandomState(2)
    x = rng.standard_normal((1, 2, 2, 4)).astype(np.float32)
    rois = np.array([[[0, 0, 1, 1], [0, 0, 1, 1], [0.2, 0.1, 0.9, 0.8], [np.nan, 0, 1, 1]]], np.float32)
    out, argmax = roi_max_pool_ref(x, rois, 7, 7, valid=[4])
    assert (argmax[0, :3] >= 0).all() and (argmax[0, 3] == -1).all() and not out[0, 3].any()
    counts = np.stack([(argmax[0, 0, :, :, 0] == p).sum() for p in range(4)])
    assert counts.sum() == 49 and counts.max() > 1
    dy = rng.standard_normal(out.shape).astype(np.float32)
    dx, dx64, n, S = roi_max_pool_backward_ref(dy, argmax, x.shape, valid=[4])
    for p in range(4):
        for c in range(4):
            chose = argmax[0, ..., c] == p
            want = dy[0, ..., c][chose].astype(np.float64).sum()
            assert n[0, p // 2, p % 2, c] == chose.sum()
            assert abs(dx64[0, p // 2, p % 2, c] - want) <= 1e-12 * max(S[0, p // 2, p % 2, c], 1.0)
    assert (np.abs(dx - dx64) <= backward_bound(n, S)).all()
    live = dy.astype(np.float64)[argmax >= 0].sum()
    assert abs(dx64.sum() - live) <= 1e-12 * np.abs(dy).sum()
    assert abs(dx.astype(np.float64).sum() - live) <= backward_bound(n, S).sum() + 1e-12 * np.abs(dy).sum()


def test_fast_restatement_is_the_scan():
    rng = np.random.RandomState(6)
    x = rng.standard_normal((2, 9, 7, 8)).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.4] = 0.0                                       # ties, and between zeros of both signs
    x[rng.uniform(size=x.shape) < 0.1] = -0.0
    x[0, 4, 3, 1], x[1, 2, 2, 5], x[1, 2, 3, 5], x[0, 1, 1, 0] = np.nan, np.nan, np.nan, -np.inf
    rois = nasty_boxes(rng, 2, 18)
    for ph, pw in ((3, 2), (7, 7), (12, 1)):
        a, b = roi_max_pool_ref(x, rois, ph, pw, valid=[18, 11]), roi_max_pool_ref(x, rois, ph, pw, valid=[18, 11], fast=True)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
        assert np.isnan(a[0]).any() and (a[0] == 0).any()


def test_nan_pixel_reaches_exactly_the_bins_that_contain_it():
    rng = np.random.RandomState(3)
    H, W = 8, 9
    x = rng.standard_normal((1, H, W, 4)).astype(np.float32)
    x[0, 3, 4, 2] = np.nan
    x[0, 6, 1, 0] = -np.inf
    rois = interior_boxes(rng, 1, 12)
    rois[0, 0] = (0, 0, 1, 1)
    out, argmax = roi_max_pool_ref(x, rois, 3, 3)
    assert not np.isnan(out[..., [0, 1, 3]]).any()
    seen = 0
    for r in range(12):
        (ylo, yhi), (xlo, xhi) = _axis(rois[0, r, 0], rois[0, r, 2], H - 1, 3, H), _axis(rois[0, r, 1], rois[0, r, 3], W - 1, 3, W)
        holds = ((ylo <= 3) & (3 < yhi))[:, None] & ((xlo <= 4) & (4 < xhi))[None, :]
        assert np.array_equal(np.isnan(out[0, r, :, :, 2]), holds)
        assert (argmax[0, r, :, :, 2][holds] == 3 * W + 4).all()
        seen += holds.sum()
    assert seen > 0


def test_dead_rows_all_box_kinds_and_valid():
    rng = np.random.RandomState(4)
    assert len(BOX_KINDS) == 9
    x = rng.standard_normal((2, 5, 9, 4)).astype(np.float32)
    rois = nasty_boxes(rng, 2, 9)
    out, argmax = roi_max_pool_ref(x, rois, 3, 4, valid=[9, 4])
    assert not np.isnan(out).any()
    for rows in (out[1, 4:], out[0, 7], out[0, 4]):                                # beyond valid, NaN box, wholly outside
        assert not rows.any() and not np.signbit(rows).any()
    assert (argmax[1, 4:] == -1).all() and (argmax[0, 7] == -1).all() and (argmax[0, 4] == -1).all()
    assert (argmax[0, [0, 1, 2, 3, 5, 6, 8]] >= 0).any(axis=(1, 2, 3)).all()       # zero-area and flipped boxes are one pixel wide
    assert (argmax[0, 5] >= 0).all() and (argmax[0, 6] >= 0).all()
    none = roi_max_pool_ref(x, rois, 3, 4, valid=[0, 0])
    assert not none[0].any() and (none[1] == -1).all()
    # a stride-exact extent moves the bins; a huge box is clamped, not overflowed
    big = np.array([[[-1e30, -np.inf, 1e30, np.inf]]], np.float32)
    o, a = roi_max_pool_ref(x[:1], big, 1, 1)
    assert np.array_equal(o[0, 0, 0, 0], x[0].reshape(-1, 4).max(axis=0))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


def _aligned(nbytes=256):
    raw = (ctypes.c_char * (nbytes + 64))()
    addr = (ctypes.addressof(raw) + 63) & ~63
    return raw, L.vp(addr)


def test_roi_max_symbols_declared_exported_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpn_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/rpn_hip.h" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
        assert getattr(lib, name).argtypes is not None


def test_roi_max_argument_validation_precedes_device_use(lib):
    _k1, x = _aligned()
    _k2, o = _aligned()
    _k3, am = _aligned()
    good = dict(B=1, H=3, W=3, C=4, R=1, ph=2, pw=2, sy=2.0, sx=2.0)

    def fwd(x=x, rois=x, out=o, argmax=None, **kw):
        a = dict(good, **kw)
        return lib.rpn_roi_max_pool(x, a["B"], a["H"], a["W"], a["C"], rois, a["R"], a["ph"], a["pw"], a["sy"], a["sx"], None, out,
                                    argmax, None)

    def bwd(dy=x, argmax=am, rois=x, dx=o, **kw):
        a = dict(good, **kw)
        return lib.rpn_roi_max_pool_backward(dy, argmax, rois, None, a["B"], a["H"], a["W"], a["C"], a["R"], a["ph"], a["pw"], a["sy"],
                                             a["sx"], dx, None)

    bad_values = [{"B": 0}, {"R": 0}, {"ph": 0}, {"pw": 0}, {"H": 0}, {"W": 0}, {"C": 6}, {"C": 0}, {"rois": None}]
    for e in (0.0, -1.0, float("nan"), float("inf")):
        bad_values += [{"sy": e}, {"sx": e}]
    for call in (fwd, bwd):
        for bad in bad_values:
            assert call(**bad) == L.RPN_ERR_INVALID, (call.__name__, bad)
            assert b"rpn_roi_max_pool" in lib.rpn_last_error()
    assert bwd(sy=float("inf")) == L.RPN_ERR_INVALID and b"extent" in lib.rpn_last_error()
    assert fwd(x=None) == L.RPN_ERR_INVALID and fwd(out=None) == L.RPN_ERR_INVALID
    assert bwd(dy=None) == L.RPN_ERR_INVALID and bwd(dx=None) == L.RPN_ERR_INVALID and bwd(argmax=None) == L.RPN_ERR_INVALID
    assert fwd(x=L.vp(x.value + 4)) == L.RPN_ERR_INVALID and b"16-byte" in lib.rpn_last_error()
    assert fwd(out=L.vp(o.value + 8)) == L.RPN_ERR_INVALID and b"16-byte" in lib.rpn_last_error()
    assert fwd(argmax=L.vp(am.value + 4)) == L.RPN_ERR_INVALID and b"16-byte" in lib.rpn_last_error()
    for arg in ("dy", "argmax", "rois", "dx"):
        assert bwd(**{arg: L.vp(x.value + 4)}) == L.RPN_ERR_INVALID and b"16-byte" in lib.rpn_last_error()
    from tf_rpn_amd.models._rpn_model import RPNModel
    m = RPNModel("vgg16", {"img_size": 96, "anchor_count": 9}, max_batch=2)

    def model(h=m._h, rois=x, B=1, R=1, ph=7, pw=7, sy=5.0, sx=5.0):
        return lib.rpn_model_roi_max_pool(h, rois, B, R, ph, pw, sy, sx, None, o, None, None)

    assert model(h=None) == L.RPN_ERR_INVALID
    assert model(B=3) == L.RPN_ERR_INVALID and b"outside [1, 2]" in lib.rpn_last_error()
    assert model(B=0) == L.RPN_ERR_INVALID and model(ph=0) == L.RPN_ERR_INVALID and model(rois=None) == L.RPN_ERR_INVALID
    assert model() == L.RPN_ERR_INVALID and b"no forward pass has run" in lib.rpn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_roi_max_compute_calls_fail_loudly_without_a_device(lib):
    _k1, x = _aligned()
    _k2, o = _aligned()
    assert lib.rpn_roi_max_pool(x, 1, 3, 3, 4, x, 1, 2, 2, 2.0, 2.0, None, o, None, None) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()
    assert lib.rpn_roi_max_pool_backward(x, x, x, None, 1, 3, 3, 4, 1, 2, 2, 2.0, 2.0, o, None) == L.RPN_ERR_NO_DEVICE
    from tf_rpn_amd.utils import roi_utils
    with pytest.raises(RuntimeError):
        roi_utils.roi_max_pooling(np.zeros((1, 3, 3, 4), np.float32), np.zeros((1, 1, 4), np.float32), (2, 2))
    with pytest.raises(RuntimeError):
        roi_utils.roi_max_pooling_backward(np.zeros((1, 1, 2, 2, 4), np.float32), np.zeros((1, 1, 2, 2, 4), np.int32),
                                           np.zeros((1, 1, 4), np.float32), (1, 3, 3, 4))


def test_roi_max_python_arguments_without_a_gpu():
    from tf_rpn_amd.models._rpn_model import FeatureExtractor, RPNModel
    from tf_rpn_amd.predictor import Proposer
    from tf_rpn_amd.utils import roi_utils
    assert callable(FeatureExtractor.roi_max_pool) and callable(RPNModel.roi_max_pool)
    x, rois = np.zeros((1, 3, 3, 4), np.float32), np.zeros((1, 1, 4), np.float32)
    for extent in ((0, 3), (3, -1), (float("nan"), 3), (3, float("inf"))):
        with pytest.raises(ValueError):
            roi_utils.roi_max_pooling(x, rois, (2, 2), extent=extent)
        with pytest.raises(ValueError):
            roi_utils.roi_max_pooling_backward(np.zeros((1, 1, 2, 2, 4), np.float32), np.zeros((1, 1, 2, 2, 4), np.int32), rois,
                                               (1, 3, 3, 4), extent=extent)
    with pytest.raises(ValueError):
        roi_utils.roi_max_pooling(x, rois, (0, 2))
    with pytest.raises(ValueError):
        roi_utils.roi_max_pooling(np.zeros((1, 3, 3, 6), np.float32), rois, (2, 2))                # C % 4 != 0
    with pytest.raises(ValueError):
        roi_utils.roi_max_pooling(np.zeros((3, 3, 4), np.float32), rois, (2, 2))
    g = np.zeros((1, 1, 2, 2, 4), np.float32)
    for argmax in (np.zeros((1, 1, 2, 2, 4), np.int64), np.zeros((1, 1, 2, 2, 4), np.float32), np.zeros((1, 1, 2, 3, 4), np.int32),
                   torch.zeros((1, 1, 2, 2, 4), dtype=torch.int64)):
        with pytest.raises(ValueError):
            roi_utils.roi_max_pooling_backward(g, argmax, rois, (1, 3, 3, 4))
    assert roi_utils._max_extent(None, 31, 31) == (30.0, 30.0) and roi_utils._max_extent(None, 1, 5) == (1.0, 4.0)
    assert default_extent(1, 5) == (1, 4)
    with pytest.raises(ValueError):
        Proposer.propose_features(None, None, pooling="maximum")          # refused before anything else is looked at


# ---- code objects ------------------------------------------------------------------------------------------------------------------
def test_roi_max_kernel_budgets(lib):
    """Register / LDS figures of the new kernels (tests/test_host.py holds every kernel of the library to no scratch).

    forward  a store waits for the (he - hs)(we - ws) pixel loads of its bin, about 20 on a large box: the kernel lives on other
             waves covering that latency, so it is held to the occupancy of roi_pool_kernel: 64 registers = eight waves per SIMD
             (a running maximum and an index per channel, one pixel in flight: nothing near that).
    backward independent waves, like roi_pool_backward_kernel: 64.
    None uses LDS, none spills."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    fwd = sorted(n for n in tab if re.match(r"roi_max_pool_kernel<[012]>$", n))
    assert fwd == ["roi_max_pool_kernel<0>", "roi_max_pool_kernel<1>", "roi_max_pool_kernel<2>"]
    for name in fwd + ["roi_max_pool_backward_kernel"]:
        vgpr, sspill, vspill, scratch, lds, wg = tab[name]
        print(name, "vgpr", vgpr, "sgpr spills", sspill, "lds", lds, "workgroup", wg)
        assert vgpr <= 64 and sspill == 0 and vspill == 0 and scratch == 0 and lds == 0, (name, vgpr, sspill, vspill, scratch, lds)
        assert wg == (64 if "backward" in name else 256)


# ---- DetectionHead.load_keras_weights: names and shapes, at the dict level ------------------------------------------------------------
def _keras_dict(fc1=(16, 8), fc2=(8, 8)):
    rng = np.random.RandomState(5)
    w = {"block5_conv3": {"kernel": rng.standard_normal((3, 3, 4, 4)).astype(np.float32), "bias": np.zeros((4,), np.float32)},
         "flatten": {},
         "fc1": {"kernel": rng.standard_normal(fc1).astype(np.float32), "bias": rng.standard_normal((fc1[1],)).astype(np.float32)},
         "fc2": {"kernel": rng.standard_normal(fc2).astype(np.float32), "bias": rng.standard_normal((fc2[1],)).astype(np.float32)},
         "predictions": {"kernel": rng.standard_normal((8, 10)).astype(np.float32), "bias": np.zeros((10,), np.float32)}}
    return w


def test_load_keras_weights_checks_names_and_shapes(lib, monkeypatch):
    from tf_rpn_amd.models.detection_head import DetectionHead
    from tf_rpn_amd.utils import h5_weights
    head = DetectionHead(3, pooling_size=(2, 2), channels=4, hidden=(8, 8), max_rois=4, seed=None)
    given = []
    monkeypatch.setattr(head, "set_weights", lambda weights, partial=False: given.append((weights, partial)) or sorted(weights))
    files = {"good": _keras_dict(), "wide": _keras_dict(fc1=(36, 8)), "narrow": _keras_dict(fc2=(8, 6))}
    files["no fc2"] = {k: v for k, v in _keras_dict().items() if k != "fc2"}
    monkeypatch.setattr(h5_weights, "read_keras_weights", lambda path: (files[path], {"layer_names": list(files[path])}))
    assert head.load_keras_weights("good") == ["fc1", "fc2"]
    (weights, partial), = given
    assert partial is True and sorted(weights) == ["fc1", "fc2"]                    # cls / reg are not touched
    for name in ("fc1", "fc2"):
        for p in ("kernel", "bias"):
            assert np.array_equal(weights[name][p], files["good"][name][p])         # as in the file: no transpose
    assert head.load_keras_weights("good", layers=("fc2",)) == ["fc2"] and sorted(given[1][0]) == ["fc2"]
    with pytest.raises(ValueError) as e:
        head.load_keras_weights("wide")
    assert "fc1" in str(e.value) and "(36, 8)" in str(e.value) and "(16, 8)" in str(e.value)
    with pytest.raises(ValueError) as e:
        head.load_keras_weights("narrow")
    assert "fc2" in str(e.value) and "(8, 6)" in str(e.value) and "(8, 8)" in str(e.value)
    assert head.load_keras_weights("narrow", layers=("fc1",)) == ["fc1"]
    with pytest.raises(ValueError) as e:
        head.load_keras_weights("no fc2")
    assert "fc2" in str(e.value)
    with pytest.raises(ValueError):
        head.load_keras_weights("good", layers=("fc1", "predictions"))
    with pytest.raises(ValueError):
        head.load_keras_weights("good", layers=("flatten",))
    assert len(given) == 3                                                          # nothing was set by the refused calls
