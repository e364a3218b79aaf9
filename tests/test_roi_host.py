"""CPU suite, RoI pooling: the numpy restatement of the contract (the oracle of tests/test_gpu_roi.py), its self-check, the C ABI
boundary without a device and the code-object figures of the new kernels.

The contract (include/rpn_hip.h, tf.image.crop_and_resize with bilinear sampling and extrapolation value 0), every operation
rounded on its own in the working dtype:
    hs = (y2 - y1) * (H - 1) / (ph - 1);  in_y(i) = y1 * (H - 1) + i * hs   (ph == 1: in_y = 0.5 * (y1 + y2) * (H - 1)); same in x
    in_y < 0, in_y > H - 1, in_x < 0, in_x > W - 1 or NaN -> 0; else t = floor(in_y), b = ceil(in_y), ly = in_y - t, l, r, lx likewise,
    top = x[t,l] + (x[t,r] - x[t,l]) * lx, bot the same on row b, out = top + (bot - top) * ly; rows r >= valid[b] are zeros.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from tf_rpn_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rpn_roi_pool", "rpn_roi_pool_backward", "rpn_model_roi_pool")


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _coords(c1, c2, n, size, dtype):
    """(n,) input coordinates of the n samples along an axis of `size` pixels under the box side [c1, c2], and which are inside."""
    span = dtype(size - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if n > 1:
            scale = (c2 - c1) * span / dtype(n - 1)
            coord = c1 * span + np.arange(n, dtype=dtype) * scale
        else:
            coord = np.full((1,), dtype(0.5) * (c1 + c2) * span, dtype=dtype)
        ok = (coord >= 0) & (coord <= span)            # False for NaN
    return coord.astype(dtype), ok


def _corners(coord, ok):
    safe = np.where(ok, coord, coord.dtype.type(0))
    lo = np.floor(safe)
    return lo.astype(np.int64), np.ceil(safe).astype(np.int64), (safe - lo).astype(coord.dtype)


def roi_pool_ref(x, rois, ph, pw, valid=None, dtype=np.float32):
    """x (B,H,W,C), rois (B,R,4) [y1,x1,y2,x2] normalised -> (B,R,ph,pw,C), all arithmetic in `dtype` (float32: the oracle)."""
    dtype = np.dtype(dtype).type
    x, rois = np.asarray(x).astype(dtype), np.asarray(rois).astype(dtype)
    B, H, W, C = x.shape
    R = rois.shape[1]
    out = np.zeros((B, R, ph, pw, C), dtype=dtype)
    for b in range(B):
        for r in range(R if valid is None else min(max(int(valid[b]), 0), R)):
            y1, x1, y2, x2 = rois[b, r]
            in_y, oky = _coords(y1, y2, ph, H, dtype)
            in_x, okx = _coords(x1, x2, pw, W, dtype)
            t, bt, ly = _corners(in_y, oky)
            l, rt, lx = _corners(in_x, okx)
            xb = x[b]
            tl, tr = xb[t[:, None], l[None, :]], xb[t[:, None], rt[None, :]]
            bl, br = xb[bt[:, None], l[None, :]], xb[bt[:, None], rt[None, :]]
            top = tl + (tr - tl) * lx[None, :, None]
            bot = bl + (br - bl) * lx[None, :, None]
            val = top + (bot - top) * ly[:, None, None]
            val[~(oky[:, None] & okx[None, :])] = 0
            out[b, r] = val
    return out


def roi_pool_backward_ref(dy, rois, shape, valid=None, coord_dtype=np.float64, unit_weights=False):
    """Scatter restatement of the adjoint, accumulated in float64: every inside sample adds dy times its four corner weights
    ((1 - ly)(1 - lx), (1 - ly) lx, ly (1 - lx), ly lx) to its corner pixels.  `coord_dtype`: the dtype the coordinates and the
    fractions are computed in.  `unit_weights`: all four weights 1 (with |dy|: the scale S of the error bound)."""
    cd = np.dtype(coord_dtype).type
    dy, rois = np.asarray(dy, dtype=np.float64), np.asarray(rois).astype(cd)
    B, H, W, C = shape
    R, ph, pw = dy.shape[1:4]
    dx = np.zeros((B, H, W, C), dtype=np.float64)
    for b in range(B):
        for r in range(R if valid is None else min(max(int(valid[b]), 0), R)):
            y1, x1, y2, x2 = rois[b, r]
            in_y, oky = _coords(y1, y2, ph, H, cd)
            in_x, okx = _coords(x1, x2, pw, W, cd)
            t, bt, ly = _corners(in_y, oky)
            l, rt, lx = _corners(in_x, okx)
            ly, lx = ly.astype(np.float64), lx.astype(np.float64)
            inside = (oky[:, None] & okx[None, :]).ravel()
            g = dy[b, r].reshape(ph * pw, C)[inside]
            for rows, wy in ((t, 1.0 - ly), (bt, ly)):
                for cols, wx in ((l, 1.0 - lx), (rt, lx)):
                    w = np.ones((ph, pw)) if unit_weights else wy[:, None] * wx[None, :]
                    yy, xx = np.broadcast_to(rows[:, None], (ph, pw)).ravel()[inside], np.broadcast_to(cols[None, :], (ph, pw)).ravel()[inside]
                    np.add.at(dx[b], (yy, xx), g * w.ravel()[inside][:, None])
    return dx


def interior_boxes(rng, B, R):
    """Corners in [0.05, 0.95], sides >= 0.02: no sample comes near the border, float32 and float64 take the same branch."""
    lo = rng.uniform(0.05, 0.93, size=(B, R, 2))
    hi = lo + rng.uniform(0.02, 1.0, size=(B, R, 2)) * (0.95 - lo - 0.02) + 0.02
    return np.concatenate([lo, np.minimum(hi, 0.95)], axis=-1).astype(np.float32)


BOX_KINDS = ("interior", "full image", "touching 1.0", "partly outside", "wholly outside", "zero area", "flipped", "NaN", "touching 0.0")


def nasty_boxes(rng, B, R, first=0, kinds=None):
    """Box (b, r) is of kind (first + b R + r) mod 9 of BOX_KINDS (or of `kinds`, a list of indices into it)."""
    kinds = list(range(len(BOX_KINDS))) if kinds is None else list(kinds)
    out = np.zeros((B, R, 4), dtype=np.float32)
    inner = interior_boxes(rng, B, R)
    for b in range(B):
        for r in range(R):
            y1, x1, y2, x2 = inner[b, r]
            kind = BOX_KINDS[kinds[(first + b * R + r) % len(kinds)]]
            out[b, r] = {
                "interior": (y1, x1, y2, x2),
                "full image": (0.0, 0.0, 1.0, 1.0),
                "touching 1.0": (y1, x1, 1.0, 1.0),
                "partly outside": (-0.2, x1, y2, 1.3),
                "wholly outside": (1.2, 1.1, 1.6, 1.5) if r % 2 else (-1.0, x1, -0.5, x2),
                "zero area": (y1, x1, y1, x1),
                "flipped": (y2, x1, y1, x2),
                "NaN": (np.nan, x1, y2, x2),
                "touching 0.0": (0.0, 0.0, y2, x2),
            }[kind]
    return out


# ---- self-check of the restatement -----------------------------------------------------------------------------------------------
def test_float32_restatement_agrees_with_float64_on_interior_boxes():
    """Bound 2e-5 * max|x|: a coordinate <= 32 computed with three roundings is off by <= 5.7e-6 pixel, and the bilinear surface's
    slope is <= 2 max|x| per pixel (measured: 6.5e-6 at max|x| = 4.5); the value's own roundings are below that."""
    rng = np.random.RandomState(0)
    for (B, H, W, C, R, ph, pw) in ((2, 31, 31, 8, 40, 7, 7), (1, 32, 32, 4, 40, 14, 14), (1, 5, 9, 4, 40, 2, 3), (1, 6, 6, 4, 20, 1, 1)):
        x = rng.standard_normal((B, H, W, C)).astype(np.float32)
        rois = interior_boxes(rng, B, R)
        assert rois.min() >= 0.05 and rois.max() <= 0.95 and (rois[..., 2:] - rois[..., :2]).min() >= 0.0199
        o32, o64 = roi_pool_ref(x, rois, ph, pw), roi_pool_ref(x, rois, ph, pw, dtype=np.float64)
        assert o32.dtype == np.float32 and o64.dtype == np.float64
        err = np.abs(o32 - o64).max()
        print("interior f32 vs f64:", (B, H, W, C, R, ph, pw), err, np.abs(x).max())
        assert err <= 2e-5 * np.abs(x).max()


def test_restatement_edge_rows_and_adjoint():
    rng = np.random.RandomState(1)
    x = rng.standard_normal((2, 5, 9, 4)).astype(np.float32)
    rois = nasty_boxes(rng, 2, 9)
    out = roi_pool_ref(x, rois, 3, 4, valid=[9, 4])
    assert not np.isnan(out).any()
    assert not out[1, 4:].any() and not out[0, 4].any() and not out[0, 7].any()      # beyond valid, wholly outside, NaN box
    assert np.array_equal(out[0, 1, 0, 0], x[0, 0, 0]) and np.array_equal(out[0, 5, 1, 2], out[0, 5, 0, 0])   # full image; zero area
    # <roi_pool(x), dy> = <x, backward(dy)> (float64 restatements of both, same float32 coordinates)
    dy = rng.standard_normal(out.shape)
    dx = roi_pool_backward_ref(dy, rois, x.shape, valid=[9, 4], coord_dtype=np.float32)
    lhs = (roi_pool_ref(x, rois, 3, 4, valid=[9, 4]).astype(np.float64) * dy).sum()
    assert abs(lhs - (x.astype(np.float64) * dx).sum()) <= 1e-5 * np.abs(dy).sum()


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


def test_roi_symbols_declared_exported_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpn_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/rpn_hip.h" % name
        assert hasattr(raw, name) and name in L.exported_symbols()
    assert "#define RPN_ABI_VERSION 1" in header and lib.rpn_abi_version() == 1


def test_roi_argument_validation_precedes_device_use(lib):
    _k1, x = _aligned()
    _k2, o = _aligned()
    good = dict(B=1, H=3, W=3, C=4, R=1, ph=2, pw=2)

    def fwd(x=x, rois=x, out=o, **kw):
        a = dict(good, **kw)
        return lib.rpn_roi_pool(x, a["B"], a["H"], a["W"], a["C"], rois, a["R"], a["ph"], a["pw"], None, out, None)

    def bwd(dy=x, rois=x, dx=o, **kw):
        a = dict(good, **kw)
        return lib.rpn_roi_pool_backward(dy, rois, None, a["B"], a["H"], a["W"], a["C"], a["R"], a["ph"], a["pw"], dx, None)

    for call in (fwd, bwd):
        for bad in ({"B": 0}, {"R": 0}, {"ph": 0}, {"pw": 0}, {"H": 0}, {"W": 0}, {"C": 6}, {"C": 0}, {"rois": None}):
            assert call(**bad) == L.RPN_ERR_INVALID, (call.__name__, bad)
            assert b"rpn_roi_pool" in lib.rpn_last_error()
    assert fwd(x=None) == L.RPN_ERR_INVALID and fwd(out=None) == L.RPN_ERR_INVALID
    assert bwd(dy=None) == L.RPN_ERR_INVALID and bwd(dx=None) == L.RPN_ERR_INVALID
    assert fwd(x=L.vp(x.value + 4)) == L.RPN_ERR_INVALID and b"16-byte" in lib.rpn_last_error()
    # the model-level entry: null handle, batch beyond max_batch, and no forward yet
    from tf_rpn_amd.models._rpn_model import RPNModel
    m = RPNModel("vgg16", {"img_size": 96, "anchor_count": 9}, max_batch=2)
    assert lib.rpn_model_roi_pool(None, x, 1, 1, 7, 7, None, o, None) == L.RPN_ERR_INVALID
    assert lib.rpn_model_roi_pool(m._h, x, 3, 1, 7, 7, None, o, None) == L.RPN_ERR_INVALID and b"outside [1, 2]" in lib.rpn_last_error()
    assert lib.rpn_model_roi_pool(m._h, x, 0, 1, 7, 7, None, o, None) == L.RPN_ERR_INVALID
    assert lib.rpn_model_roi_pool(m._h, x, 1, 1, 0, 7, None, o, None) == L.RPN_ERR_INVALID
    assert lib.rpn_model_roi_pool(m._h, None, 1, 1, 7, 7, None, o, None) == L.RPN_ERR_INVALID
    assert lib.rpn_model_roi_pool(m._h, x, 1, 1, 7, 7, None, o, None) == L.RPN_ERR_INVALID and b"no forward pass has run" in lib.rpn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_roi_compute_calls_fail_loudly_without_a_device(lib):
    _k1, x = _aligned()
    _k2, o = _aligned()
    assert lib.rpn_roi_pool(x, 1, 3, 3, 4, x, 1, 2, 2, None, o, None) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()
    assert lib.rpn_roi_pool_backward(x, x, None, 1, 3, 3, 4, 1, 2, 2, o, None) == L.RPN_ERR_NO_DEVICE
    from tf_rpn_amd.utils import roi_utils
    with pytest.raises(RuntimeError):
        roi_utils.roi_pooling(np.zeros((1, 3, 3, 4), np.float32), np.zeros((1, 1, 4), np.float32), (2, 2))


def test_roi_utils_imports_without_a_gpu():
    from tf_rpn_amd.utils import roi_utils
    assert callable(roi_utils.roi_pooling) and callable(roi_utils.roi_pooling_backward)
    assert "no counterpart in the reference" in roi_utils.__doc__.lower()
    with pytest.raises(ValueError):
        roi_utils._pool_size((0, 7))
    from tf_rpn_amd.models._rpn_model import FeatureExtractor
    from tf_rpn_amd.predictor import Proposer
    assert callable(FeatureExtractor.roi_pool) and callable(Proposer.propose_features)


# ---- code objects ------------------------------------------------------------------------------------------------------------------
def test_roi_kernel_budgets(lib):
    """Register / LDS figures of the new kernels (budgets of their own; tests/test_host.py holds every kernel of the library to no
    scratch).  The forward is store-bound and hides its corner loads behind other waves: 64 registers = eight waves per SIMD, in
    all three instantiations (float32 NHWC, split bfloat16, split float16); the backward's waves are independent, 64 likewise.
    Neither uses LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    fwd = {n: r for n, r in tab.items() if re.match(r"roi_pool_kernel<[012]>$", n)}
    assert sorted(fwd) == ["roi_pool_kernel<0>", "roi_pool_kernel<1>", "roi_pool_kernel<2>"]
    assert "roi_pool_backward_kernel" in tab
    for name, (vgpr, sspill, vspill, scratch, lds, wg) in list(fwd.items()) + [("roi_pool_backward_kernel", tab["roi_pool_backward_kernel"])]:
        print(name, "vgpr", vgpr, "sgpr spills", sspill, "lds", lds, "workgroup", wg)
        assert vgpr <= 64 and sspill == 0 and vspill == 0 and scratch == 0 and lds == 0, (name, vgpr, sspill, vspill, scratch, lds)
        assert wg == (64 if "backward" in name else 256)
