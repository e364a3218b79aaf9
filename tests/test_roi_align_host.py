"""CPU suite, RoI Align: the numpy restatement of the contract (the oracle of tests/test_gpu_roi_align.py), its self-checks against
float64 and against two known answers, the C ABI boundary without a device and the code-object figures of the new kernels.

The contract (include/rpn_hip.h), every operation rounded on its own in the working dtype, per axis (y shown):
    start = y1 * Sy - 0.5;  end = y2 * Sy - 0.5;  bin = (end - start) / ph;  step = bin / s
    sample k of bin i:  y = (start + i * bin) + (k + 0.5) * step;  ok = y >= -1 && y <= H (false for NaN)
    if (y < 0) y = 0;  lo = (int)y;  if (lo >= H - 1) { lo = hi = H - 1; y = lo; } else hi = lo + 1;  l = y - lo;  h = 1 - l
    sample = ((hy*hx * x[lo_y,lo_x] + hy*lx * x[lo_y,hi_x]) + ly*hx * x[hi_y,lo_x]) + ly*lx * x[hi_y,hi_x]
    out = (the ok samples added to +0 in (ky, kx) order) / (s * s); rows r >= valid[b] are zeros.

The coordinate bound the tolerances below are built on: a coordinate is the result of at most 9 rounded float32 operations
(y1 * Sy, - 0.5, the same two for `end` feed one subtraction, / ph, / s, i * bin, start + ., (k + 0.5) * step, the last +) on
quantities below 32 on a map up to 32 wide (below 64 up to 64 wide).  Each rounds by at most half an ulp of a number below 32,
2^-20 = 9.5e-7 pixel; bin and step errors are multiplied by i < ph and (k + 0.5) < s, but i * bin and (k + 0.5) * step are
themselves below 32, so no term carries more than the relative error of the operations before it: 9 * 2^-20 * (1 + a few 2^-24)
<= 1.72e-5 pixel = COORD_EPS for maps up to 32, twice that up to 64.
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
SYMBOLS = ("rpn_roi_align", "rpn_roi_align_backward", "rpn_model_roi_align")
COORD_EPS = 1.72e-5                     # pixels, maps up to 32 wide (module docstring)


def coord_eps(H, W):
    assert max(H, W) <= 64
    return COORD_EPS * (1 if max(H, W) <= 32 else 2)


def f32_vs_f64_bound(H, W):
    """|float32 result - float64 result| / max|x| (test_float32_restatement_agrees_with_float64 derives it)"""
    return 2 * coord_eps(H, W) + 21 * 2.0 ** -24


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _axis(c1, c2, extent, n, s, size, dtype):
    """-> lo, hi (n, s) int64 pixels, l, h (n, s) weights of hi / lo in `dtype`, ok (n, s): the s samples of each of the n bins."""
    half, zero = dtype(0.5), dtype(0)
    with np.errstate(invalid="ignore", over="ignore"):
        start, end = c1 * extent - half, c2 * extent - half
        bin_ = (end - start) / dtype(n)
        step = bin_ / dtype(s)
        i, k = np.arange(n, dtype=dtype)[:, None], np.arange(s, dtype=dtype)[None, :]
        y = ((start + i * bin_) + (k + half) * step).astype(dtype)
        ok = (y >= dtype(-1)) & (y <= dtype(size))          # False for NaN
        y = np.where(ok, y, zero)
        y = np.where(y < zero, zero, y)
        lo = y.astype(np.int64)
        top = lo >= size - 1
        lo = np.where(top, size - 1, lo)
        hi = np.where(top, size - 1, lo + 1)
        y = np.where(top, lo.astype(dtype), y)
        l = (y - lo.astype(dtype)).astype(dtype)
        h = (dtype(1) - l).astype(dtype)
    return lo, hi, l, h, ok


def _extent(extent, H, W, dtype):
    sy, sx = (H, W) if extent is None else extent
    return dtype(np.float32(sy)), dtype(np.float32(sx))      # the ABI takes float32


def _live(valid, b, R):
    return R if valid is None else min(max(int(valid[b]), 0), R)


def roi_align_ref(x, rois, ph, pw, s, extent=None, valid=None, dtype=np.float32):
    """x (B,H,W,C), rois (B,R,4) [y1,x1,y2,x2] normalised -> (B,R,ph,pw,C), all arithmetic in `dtype` (float32: the oracle)."""
    dtype = np.dtype(dtype).type
    x, rois = np.asarray(x).astype(dtype), np.asarray(rois).astype(dtype)
    B, H, W, C = x.shape
    R = rois.shape[1]
    sy, sx = _extent(extent, H, W, dtype)
    out = np.zeros((B, R, ph, pw, C), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            xb = x[b]
            for r in range(_live(valid, b, R)):
                y1, x1, y2, x2 = rois[b, r]
                ylo, yhi, ly, hy, oky = _axis(y1, y2, sy, ph, s, H, dtype)
                xlo, xhi, lx, hx, okx = _axis(x1, x2, sx, pw, s, W, dtype)
                acc = np.zeros((ph, pw, C), dtype=dtype)
                for ky in range(s):
                    for kx in range(s):
                        t, bt, l, rt = ylo[:, ky, None], yhi[:, ky, None], xlo[None, :, kx], xhi[None, :, kx]
                        wy_h, wy_l, wx_h, wx_l = hy[:, ky, None], ly[:, ky, None], hx[None, :, kx], lx[None, :, kx]
                        w1, w2, w3, w4 = (wy_h * wx_h)[..., None], (wy_h * wx_l)[..., None], (wy_l * wx_h)[..., None], (wy_l * wx_l)[..., None]
                        val = ((w1 * xb[t, l] + w2 * xb[t, rt]) + w3 * xb[bt, l]) + w4 * xb[bt, rt]
                        ok = (oky[:, ky, None] & okx[None, :, kx])[..., None]
                        acc = (acc + np.where(ok, val, dtype(0))).astype(dtype)
                out[b, r] = acc / dtype(s * s)
    return out


def _axis_matrix(lo, hi, l, h, ok, size):
    """A (n, size) float64: A[i, p] = the summed weight pixel p has in bin i"""
    n, s = lo.shape
    A = np.zeros((n, size), dtype=np.float64)
    rows = np.arange(n)
    for k in range(s):
        np.add.at(A, (rows, lo[:, k]), np.where(ok[:, k], h[:, k].astype(np.float64), 0.0))
        np.add.at(A, (rows, hi[:, k]), np.where(ok[:, k], l[:, k].astype(np.float64), 0.0))
    return A


def roi_align_backward_ref(dy, rois, shape, s, extent=None, valid=None, coord_dtype=np.float64, unit_weights=False):
    """Scatter restatement of the adjoint, accumulated in float64: bin (i, j) adds dy * Ay(i, py) * Ax(j, px) / (s * s) to pixel
    (py, px).  `coord_dtype`: the dtype the coordinates and the fractions are computed in.  `unit_weights`: every non-zero axis
    weight Ay, Ax is 1 and nothing is divided (with |dy|: the scale S of the error bound)."""
    cd = np.dtype(coord_dtype).type
    dy, rois = np.asarray(dy, dtype=np.float64), np.asarray(rois).astype(cd)
    B, H, W, C = shape
    R, ph, pw = dy.shape[1:4]
    sy, sx = _extent(extent, H, W, cd)
    dx = np.zeros((B, H, W, C), dtype=np.float64)
    for b in range(B):
        for r in range(_live(valid, b, R)):
            y1, x1, y2, x2 = rois[b, r]
            Ay = _axis_matrix(*_axis(y1, y2, sy, ph, s, H, cd), H)
            Ax = _axis_matrix(*_axis(x1, x2, sx, pw, s, W, cd), W)
            if unit_weights:
                Ay, Ax = (Ay != 0).astype(np.float64), (Ax != 0).astype(np.float64)
            else:
                Ay = Ay / (s * s)
            dx[b] += np.tensordot(Ax, np.tensordot(Ay, dy[b, r], axes=(0, 0)), axes=(0, 1)).transpose(1, 0, 2)   # ih,jw,ijc->hwc
    return dx


ISSUE_CASES = [(2, 31, 31, 8, 40, 7, 7, 2), (1, 32, 32, 4, 40, 14, 14, 1), (1, 5, 9, 4, 40, 2, 3, 3), (1, 6, 6, 4, 20, 1, 1, 4),
               (1, 63, 63, 4, 40, 7, 7, 2)]


# ---- self-checks of the restatement ---------------------------------------------------------------------------------------------
def test_float32_restatement_agrees_with_float64():
    """Bound f32_vs_f64_bound = (2 * COORD_EPS + 21 u) max|x|, u = 2^-24: the float32 coordinate is within COORD_EPS of the
    float64 one (module docstring), the bilinear surface has a slope of at most 2 max|x| per pixel, and the value's own roundings
    stay within (5 + s * s) u max|x| <= 21 u max|x| (affine_bound counts them): 3.6e-5 max|x| on maps up to 32 wide, 7e-5 on maps
    of 33 to 64.  (Both axes attaining the worst slope AND the worst rounding at once would double it;
    that needs a +-max|x| checkerboard under a sample whose nine operations all round the same way on both axes, and the
    tighter figure is the one held.)  The average of s * s samples obeys the bound of one.  On boxes inside [0, 1] no sample is
    within half a pixel of an ok threshold, so both precisions keep the same samples.  (A scratch restatement measured at most
    3.1e-6 max|x|.)"""
    rng = np.random.RandomState(0)
    for (B, H, W, C, R, ph, pw, s) in ISSUE_CASES:
        x = rng.standard_normal((B, H, W, C)).astype(np.float32)
        for rois in (interior_boxes(rng, B, R), np.clip(nasty_boxes(rng, B, R, kinds=[0, 1, 2, 8, 5]), 0, 1)):
            o32, o64 = roi_align_ref(x, rois, ph, pw, s), roi_align_ref(x, rois, ph, pw, s, dtype=np.float64)
            assert o32.dtype == np.float32 and o64.dtype == np.float64
            err, mx = np.abs(o32 - o64).max(), np.abs(x).max()
            print("align f32 vs f64:", (B, H, W, C, R, ph, pw, s), err, mx)
            assert err <= f32_vs_f64_bound(H, W) * mx


@pytest.mark.parametrize("n", [4, 7, 31, 32])
def test_identity_known_answer(n):
    """Box [0,0,1,1], ph = pw = H = W, s = 1, default extent: start = -0.5, end = n - 0.5, bin = 1 exactly, so sample i is pixel
    centre i exactly, l = 0, and the output is x[0] bit for bit (1 * x + 0 * neighbours; the data has no zeros or non-finites)."""
    rng = np.random.RandomState(n)
    x = rng.standard_normal((1, n, n, 4)).astype(np.float32)
    out = roi_align_ref(x, np.array([[[0, 0, 1, 1]]], np.float32), n, n, 1)
    assert np.array_equal(out[0, 0].view(np.uint32), x[0].view(np.uint32))


def affine_case():
    """-> x (1,31,29,4), rois (1,50,4), want(s) (1,50,7,5,4) float64: the affine map's value at every bin centre"""
    rng = np.random.RandomState(3)
    H, W, a, b, c0 = 31, 29, 0.375, -1.25, 2.0
    x = (a * np.arange(H)[:, None] + b * np.arange(W)[None, :] + c0)[None, :, :, None].repeat(4, axis=3).astype(np.float32)
    lo = rng.uniform(0.05, 0.5, size=(1, 50, 2))
    rois = np.concatenate([lo, lo + rng.uniform(0.05, 0.44, size=(1, 50, 2))], axis=-1).astype(np.float32)
    r64 = rois.astype(np.float64)
    cy = r64[..., 0, None] * H - 0.5 + (np.arange(7) + 0.5) * ((r64[..., 2] - r64[..., 0]) * H / 7)[..., None]       # (1,50,7)
    cx = r64[..., 1, None] * W - 0.5 + (np.arange(5) + 0.5) * ((r64[..., 3] - r64[..., 1]) * W / 5)[..., None]       # (1,50,5)
    assert cy.min() - 0.5 * 0.44 * H / 7 >= 0 and cy.max() + 0.5 * 0.44 * H / 7 <= H - 1        # every sample inside [0, H - 1]
    assert cx.min() - 0.5 * 0.44 * W / 5 >= 0 and cx.max() + 0.5 * 0.44 * W / 5 <= W - 1
    want = (a * cy[..., :, None] + b * cx[..., None, :] + c0)[..., None].repeat(4, axis=-1)
    return x, rois, want, (a, b)


def affine_bound(x, ab, s):
    """COORD_EPS * (|a| + |b|) + (6 + s * s) u max|x|, u = 2^-24: a bilinear sample of an affine map IS the map at the sample,
    the samples of a bin average to the bin centre, and each sample coordinate is off by <= COORD_EPS.  The value's own
    roundings: a sample is four terms of two rounded products each and three sums, <= 5 u max|x| (the weights add up to 1); the
    s * s - 1 sums of the bin round partial sums below s * s max|x|, and the division takes that back: <= (s * s - 1) u max|x|;
    the division itself and x's own rounding to float32 one u each."""
    return COORD_EPS * (abs(ab[0]) + abs(ab[1])) + (6 + s * s) * 2.0 ** -24 * np.abs(x).max()


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_affine_known_answer(s):
    x, rois, want, ab = affine_case()
    err = np.abs(roi_align_ref(x, rois, 7, 5, s) - want).max()
    print("affine known answer: s", s, "err", err, "max|x|", np.abs(x).max(), "bound", affine_bound(x, ab, s))
    assert err <= affine_bound(x, ab, s)


def test_restatement_edge_rows_and_adjoint():
    """All nine box kinds with `valid`: no NaN leaves the operator, dead rows are zeros, and <align(x), dy> = <x, backward(dy)> for
    the float64 restatements of both on the same float32 coordinates."""
    rng = np.random.RandomState(1)
    assert len(BOX_KINDS) == 9
    x = rng.standard_normal((2, 5, 9, 4)).astype(np.float32)
    rois = nasty_boxes(rng, 2, 9)
    for s in (1, 2, 3):
        out = roi_align_ref(x, rois, 3, 4, s, valid=[9, 4])
        assert not np.isnan(out).any()
        assert not out[1, 4:].any() and not out[0, 7].any()                       # beyond valid, NaN box
        assert not out[0, 4].any()                                                # wholly outside: further than one pixel
        dy = rng.standard_normal(out.shape)
        dx = roi_align_backward_ref(dy, rois, x.shape, s, valid=[9, 4], coord_dtype=np.float32)
        # the forward in float64 VALUES on float32 COORDINATES is linear in x with exactly the backward's weights
        lhs = (_forward64_on_f32_coords(x, rois, 3, 4, s, [9, 4]) * dy).sum()
        rhs = (x.astype(np.float64) * dx).sum()
        assert abs(lhs - rhs) <= 1e-12 * np.abs(dy).sum() * np.abs(x).max()
        # ... and the sample-by-sample float32 forward, written independently of the axis matrices, is that operator to rounding
        assert abs((out.astype(np.float64) * dy).sum() - rhs) <= 1e-5 * np.abs(dy).sum()


def _forward64_on_f32_coords(x, rois, ph, pw, s, valid):
    B, H, W, C = x.shape
    out = np.zeros((B, rois.shape[1], ph, pw, C))
    for b in range(B):
        for r in range(_live(valid, b, rois.shape[1])):
            y1, x1, y2, x2 = rois[b, r]
            Ay = _axis_matrix(*_axis(y1, y2, np.float32(H), ph, s, H, np.float32), H)
            Ax = _axis_matrix(*_axis(x1, x2, np.float32(W), pw, s, W, np.float32), W)
            out[b, r] = np.einsum("ih,jw,hwc->ijc", Ay, Ax, x[b].astype(np.float64), optimize=True) / (s * s)
    return out


def test_separable_forward_matches_the_sample_by_sample_restatement():
    """The two restatements are written independently (samples one by one / separable axis matrices): they agree to rounding."""
    rng = np.random.RandomState(2)
    x = rng.standard_normal((2, 6, 7, 4)).astype(np.float32)
    rois = nasty_boxes(rng, 2, 9)
    for s in (1, 2, 4):
        a = roi_align_ref(x, rois, 3, 2, s, valid=[9, 5])
        assert np.abs(a - _forward64_on_f32_coords(x, rois, 3, 2, s, [9, 5])).max() <= 16 * 2.0 ** -24 * np.abs(x).max()


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


def test_roi_align_symbols_declared_exported_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpn_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/rpn_hip.h" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
        assert getattr(lib, name).argtypes is not None


def test_roi_align_argument_validation_precedes_device_use(lib):
    _k1, x = _aligned()
    _k2, o = _aligned()
    good = dict(B=1, H=3, W=3, C=4, R=1, ph=2, pw=2, s=2, sy=3.0, sx=3.0)

    def fwd(x=x, rois=x, out=o, **kw):
        a = dict(good, **kw)
        return lib.rpn_roi_align(x, a["B"], a["H"], a["W"], a["C"], rois, a["R"], a["ph"], a["pw"], a["s"], a["sy"], a["sx"], None,
                                 out, None)

    def bwd(dy=x, rois=x, dx=o, **kw):
        a = dict(good, **kw)
        return lib.rpn_roi_align_backward(dy, rois, None, a["B"], a["H"], a["W"], a["C"], a["R"], a["ph"], a["pw"], a["s"], a["sy"],
                                          a["sx"], dx, None)

    bad_values = [{"B": 0}, {"R": 0}, {"ph": 0}, {"pw": 0}, {"H": 0}, {"W": 0}, {"C": 6}, {"C": 0}, {"rois": None},
                  {"s": 0}, {"s": -1}, {"s": 5}]
    for e in (0.0, -1.0, float("nan"), float("inf")):
        bad_values += [{"sy": e}, {"sx": e}]
    for call in (fwd, bwd):
        for bad in bad_values:
            assert call(**bad) == L.RPN_ERR_INVALID, (call.__name__, bad)
            assert b"rpn_roi_align" in lib.rpn_last_error()
    assert fwd(s=5) == L.RPN_ERR_INVALID and b"sampling_ratio" in lib.rpn_last_error()
    assert bwd(sy=float("inf")) == L.RPN_ERR_INVALID and b"extent" in lib.rpn_last_error()
    assert fwd(x=None) == L.RPN_ERR_INVALID and fwd(out=None) == L.RPN_ERR_INVALID
    assert bwd(dy=None) == L.RPN_ERR_INVALID and bwd(dx=None) == L.RPN_ERR_INVALID
    assert fwd(x=L.vp(x.value + 4)) == L.RPN_ERR_INVALID and b"16-byte" in lib.rpn_last_error()
    assert fwd(out=L.vp(o.value + 8)) == L.RPN_ERR_INVALID and b"16-byte" in lib.rpn_last_error()
    for arg in ("dy", "rois", "dx"):
        assert bwd(**{arg: L.vp(x.value + 4)}) == L.RPN_ERR_INVALID and b"16-byte" in lib.rpn_last_error()
    # the model-level entry: null handle, batch beyond max_batch, bad sampling, and no forward yet
    from tf_rpn_amd.models._rpn_model import RPNModel
    m = RPNModel("vgg16", {"img_size": 96, "anchor_count": 9}, max_batch=2)

    def model(h=m._h, rois=x, B=1, R=1, ph=7, pw=7, s=2, sy=6.0, sx=6.0):
        return lib.rpn_model_roi_align(h, rois, B, R, ph, pw, s, sy, sx, None, o, None)

    assert model(h=None) == L.RPN_ERR_INVALID
    assert model(B=3) == L.RPN_ERR_INVALID and b"outside [1, 2]" in lib.rpn_last_error()
    assert model(B=0) == L.RPN_ERR_INVALID and model(ph=0) == L.RPN_ERR_INVALID and model(rois=None) == L.RPN_ERR_INVALID
    assert model() == L.RPN_ERR_INVALID and b"no forward pass has run" in lib.rpn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_roi_align_compute_calls_fail_loudly_without_a_device(lib):
    _k1, x = _aligned()
    _k2, o = _aligned()
    assert lib.rpn_roi_align(x, 1, 3, 3, 4, x, 1, 2, 2, 2, 3.0, 3.0, None, o, None) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()
    assert lib.rpn_roi_align_backward(x, x, None, 1, 3, 3, 4, 1, 2, 2, 2, 3.0, 3.0, o, None) == L.RPN_ERR_NO_DEVICE
    from tf_rpn_amd.utils import roi_utils
    with pytest.raises(RuntimeError):
        roi_utils.roi_align(np.zeros((1, 3, 3, 4), np.float32), np.zeros((1, 1, 4), np.float32), (2, 2))
    with pytest.raises(RuntimeError):
        roi_utils.roi_align_backward(np.zeros((1, 1, 2, 2, 4), np.float32), np.zeros((1, 1, 4), np.float32), (1, 3, 3, 4))


def test_roi_align_python_arguments_without_a_gpu():
    from tf_rpn_amd.models._rpn_model import FeatureExtractor, RPNModel
    from tf_rpn_amd.predictor import Proposer
    from tf_rpn_amd.utils import roi_utils
    assert callable(roi_utils.roi_align) and callable(roi_utils.roi_align_backward)
    assert callable(FeatureExtractor.roi_align) and callable(RPNModel.roi_align)
    x, rois = np.zeros((1, 3, 3, 4), np.float32), np.zeros((1, 1, 4), np.float32)
    for s in (0, -1, 5, 1.5):
        with pytest.raises(ValueError):
            roi_utils.roi_align(x, rois, (2, 2), sampling_ratio=s)
        with pytest.raises(ValueError):
            roi_utils.roi_align_backward(np.zeros((1, 1, 2, 2, 4), np.float32), rois, (1, 3, 3, 4), sampling_ratio=s)
    for extent in ((0, 3), (3, -1), (float("nan"), 3), (3, float("inf"))):
        with pytest.raises(ValueError):
            roi_utils.roi_align(x, rois, (2, 2), extent=extent)
    with pytest.raises(ValueError):
        roi_utils.roi_align(x, rois, (0, 2))
    with pytest.raises(ValueError):
        Proposer.propose_features(None, None, pooling="max")              # refused before anything else is looked at


# ---- code objects ------------------------------------------------------------------------------------------------------------------
def test_roi_align_kernel_budgets(lib):
    """Register / LDS figures of the new kernels (tests/test_host.py holds every kernel of the library to no scratch).

    forward  At s = 2 a store waits for 16 corner loads, at s = 4 for 64: the kernel lives on other waves covering that latency,
             so it is held to the occupancy of roi_pool_kernel or one step below it.  float32 source: 64 registers = eight
             waves per SIMD.  Split sources: a sample has eight 8-byte loads in flight (hi and lo halves of four corners) and
             joins them into the same four float4, beside the four kept sample columns: 80 registers = six waves per SIMD
             (512 / 80), the next allocation step above 64 + the eight registers the joins need.
    backward independent waves, like roi_pool_backward_kernel: 64.
    None uses LDS, none spills."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    fwd = {n: r for n, r in tab.items() if re.match(r"roi_align_kernel<[012]>$", n)}
    assert sorted(fwd) == ["roi_align_kernel<0>", "roi_align_kernel<1>", "roi_align_kernel<2>"]
    assert "roi_align_backward_kernel" in tab
    budget = {"roi_align_kernel<0>": 64, "roi_align_kernel<1>": 80, "roi_align_kernel<2>": 80, "roi_align_backward_kernel": 64}
    for name, limit in budget.items():
        vgpr, sspill, vspill, scratch, lds, wg = tab[name]
        print(name, "vgpr", vgpr, "sgpr spills", sspill, "lds", lds, "workgroup", wg)
        assert vgpr <= limit and sspill == 0 and vspill == 0 and scratch == 0 and lds == 0, (name, vgpr, sspill, vspill, scratch, lds)
        assert wg == (64 if "backward" in name else 256)
    for name in ("roi_pool_kernel<0>", "roi_pool_kernel<1>", "roi_pool_kernel<2>", "roi_pool_backward_kernel"):
        assert name in tab
