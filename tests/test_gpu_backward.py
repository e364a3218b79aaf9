"""The backward kernels of the training path, one layer at a time, through the public single-layer entries (rpn_conv3x3_dgrad,
rpn_conv3x3_wgrad_wide, rpn_conv3x3_wgrad, rpn_maxpool2x2_backward): real values against float64, H != W, every tile path and the
channel / size edges the ABI accepts, every device buffer inside guard bands.

References: the float64 numpy restatements of tests/test_train_backbone.py (dgrad64, wgrad64, maxpool_backward64) and, as a second
oracle written independently of them, torch.nn.grad.conv2d_input / conv2d_weight and autograd through F.max_pool2d in float64 on
the CPU; test_references_agree_* hold the two against each other without a GPU.  The activations are inputs here, so the reference
sees the same ReLU masks and pool maxima as the kernel: the bound is float32 rounding, not the 5e-3 of the whole-model test.

Guard bands: every input, output and workspace is a view into a larger device buffer filled with a NaN canary (4096 floats on both
sides; the workspace view exactly *_workspace_bytes long and itself full of canary).  A store outside a buffer changes canary
bits, a read outside one (or of workspace nobody wrote) that enters a sum turns the output NaN, an output element nobody wrote
stays NaN.

Parity bound (test_*_real_values_*): err(t) = max|t - ref64| / max|ref64|; e32 = err of a plain float32 evaluation of the same
operation on the CPU (numpy, float32 matmuls); asserted err(gpu) <= MARGIN * max(e32, 2^-24) and, element-wise, the rigorous
|t - ref64| <= (K + depth) 2^-24 (|A| |B|).  MARGIN covers the difference between two correct float32 summation orders only; see
the comment at MARGIN for the experiment behind its value.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry  # noqa: E402
from test_train_backbone import dgrad64, maxpool_backward64, wgrad64  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402

U = 2.0 ** -24                  # unit roundoff of float32
# MARGIN: how far two CORRECT float32 summation orders lie apart under the metric above.  Measured on the CPU alone, with the data
# builders below: a strictly sequential fmaf chain (what v_mfma_f32_32x32x2_f32 computes; also with K slices of 2) against numpy's
# blocked float32 matmul, both against float64, as chain / max(e32, 2^-24), worst of 8 seeds (100-200 for the tiny cases):
#   sum length 576 (dgrad, Cout 64) 1.8   4608 (dgrad, Cout 512) 5.9   16 (one pixel, Cout 16) 4.2   144 (15 pixels, Cout 16) 6.6
#   1000 pixels per leaf (wgrad_wide) 2.5   16 000 pixels per leaf (wgrad) 14.2   db: 1000 pixels 5.2, 16 000 pixels 4.3
# The chain's error grows like sqrt(K), the blocked sum's hardly at all, so 8 does not cover the long sums; 16 covers the worst
# spread seen.  The same experiment with one operand rounded through float16 gives at least 247 (K = 16) and 450 - 1400 elsewhere
# times max(e32, 2^-24): a 16-bit operand path fails by a factor of 15 or more.
MARGIN = 16.0
GUARD = 4096                    # floats of canary on each side of every device buffer
CANARY = 0x7FC0BEEF             # a quiet NaN with a payload: arithmetic on it gives NaN, a store over it changes its bits


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


# ---- shape tables (test_shape_tables_reach_every_path classifies them with the library's own host functions) -------------------------
# (B, H, W, Cin, Cout).  H != W unless the shape restates a VGG16 layer.
DGRAD = [(1, 1, 1, 4, 16), (1, 3, 5, 4, 16), (2, 7, 13, 20, 48), (1, 9, 33, 68, 16),
         (3, 31, 17, 132, 80),            # 64-wide tile, ragged: 132 = 2 * 64 + 4
         (1, 40, 23, 192, 48),
         (2, 250, 131, 128, 128),         # 128-wide tile at exactly 512 tiles
         (4, 125, 97, 320, 64),           # 128-wide tile, ragged: 320 = 2 * 128 + 64
         (8, 250, 250, 128, 128), (8, 125, 125, 256, 256)]      # block2_conv2 / block3_conv2 at the benchmarked batch
WGRAD_WIDE = [(1, 1, 1, 3, 4), (1, 3, 5, 4, 20),
              (1, 15, 15, 512, 512),      # one leaf: block 5 at 250 x 250
              (1, 40, 27, 12, 132),       # two leaves: the tree loop skipped
              (2, 62, 31, 256, 132), (2, 62, 47, 128, 68), (1, 250, 131, 64, 128),
              (2, 500, 500, 3, 64),       # block1_conv1, 512 leaves
              (1, 500, 333, 64, 64)]
WGRAD_HEAD = [(1, 1, 1, 4, 4), (1, 1, 2, 4, 4),                # fewer pixels than the four leaves
              (2, 7, 5, 20, 36), (1, 9, 33, 64, 132), (3, 31, 17, 512, 512), (8, 31, 31, 512, 512)]
POOL = [(1, 2, 2, 4), (2, 3, 2, 4), (1, 7, 10, 8), (3, 10, 7, 68), (2, 125, 62, 256), (1, 500, 333, 64)]      # (B, H, W, C)


def a256(n):
    return (n + 255) & ~255


def wide_leaves(lib, B, H, W, Cin, Cout):
    """The number of pixel ranges (leaves) rpn_conv3x3_wgrad_wide splits a shape into, recovered from its workspace size:
    bytes = a256(L * slab) + pad, slab = (9 cin_x + 1) Cout floats (cin_x = Cin rounded up to 4: nine taps and the row of ones
    behind db), pad = a256(B H W * 4 floats) for the image padded to four channels when Cin == 3, else 0.  A slab is at least
    (9 * 4 + 1) * 4 floats = 592 bytes > 256, so a256(L * slab) grows strictly with L and the power of two is unique."""
    total = lib.rpn_conv3x3_wgrad_wide_workspace_bytes(B, H, W, Cin, Cout)
    cin_x = (Cin + 3) // 4 * 4
    slab = (9 * cin_x + 1) * Cout * 4
    pad = a256(B * H * W * 4 * 4) if Cin == 3 else 0
    found = [n for n in (1 << k for k in range(11)) if a256(n * slab) + pad == total]
    assert len(found) == 1, (B, H, W, Cin, Cout, total)
    return found[0]


# ---- data shaped like what the trainer feeds ----------------------------------------------------------------------------------------------
def dy_like(rng, shape):
    """ReLU-masked gradients: about half the entries exactly zero, the others spread over three decades."""
    v = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 0.0, size=shape)
    v[rng.uniform(size=shape) < 0.5] = 0.0
    return v.astype(np.float32)


def relu_like(rng, shape):
    return np.maximum(rng.standard_normal(shape), 0.0).astype(np.float32)


def he_like(rng, Cin, Cout):
    return (rng.standard_normal((3, 3, Cin, Cout)) * math.sqrt(2.0 / (9 * Cin))).astype(np.float32)


# ---- plain float32 evaluations on the CPU (the yardstick e32 of the parity bound) ------------------------------------------------------
def dgrad32(dy, w):
    B, H, W, Cout = dy.shape
    dyp = np.zeros((B, H + 2, W + 2, Cout), np.float32)
    dyp[:, 1:H + 1, 1:W + 1] = dy
    dx = np.zeros((B, H, W, w.shape[2]), np.float32)
    for r in range(3):
        for s in range(3):
            dx += dyp[:, 2 - r:2 - r + H, 2 - s:2 - s + W] @ w[r, s].T
    assert dx.dtype == np.float32
    return dx


def wgrad32(x, dy):
    B, H, W, Cin = x.shape
    xp = np.zeros((B, H + 2, W + 2, Cin), np.float32)
    xp[:, 1:H + 1, 1:W + 1] = x
    d2 = dy.reshape(-1, dy.shape[3])
    dw = np.zeros((3, 3, Cin, dy.shape[3]), np.float32)
    for r in range(3):
        for s in range(3):
            dw[r, s] = xp[:, r:r + H, s:s + W].reshape(-1, Cin).T @ d2
    db = (np.ones((1, d2.shape[0]), np.float32) @ d2)[0]          # db as the kernels form it: one more row of the GEMM
    assert dw.dtype == np.float32 and db.dtype == np.float32
    return dw, db


# ---- the second float64 oracle: torch on the CPU ----------------------------------------------------------------------------------------
def nchw64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 3, 1, 2)


def dgrad_torch(dy, w):
    B, H, W, _ = dy.shape
    k = torch.from_numpy(np.ascontiguousarray(w, np.float64)).permute(3, 2, 0, 1)            # HWIO -> OIHW
    dx = torch.nn.grad.conv2d_input((B, w.shape[2], H, W), k, nchw64(dy), padding=1)
    return dx.permute(0, 2, 3, 1).numpy()


def wgrad_torch(x, dy):
    g = nchw64(dy)
    dw = torch.nn.grad.conv2d_weight(nchw64(x), (dy.shape[3], x.shape[3], 3, 3), g, padding=1)
    return dw.permute(2, 3, 1, 0).numpy(), g.sum((0, 2, 3)).numpy()


def maxpool_backward_torch(y, dpool):
    t = nchw64(y).clone().requires_grad_(True)
    torch.relu(torch.nn.functional.max_pool2d(t, 2, 2)).backward(nchw64(dpool))
    return t.grad.permute(0, 2, 3, 1).numpy()


# ---- CPU: the references judge each other before they judge a kernel ---------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 1, 1, 4, 16), (2, 3, 5, 4, 16), (1, 7, 4, 12, 32), (3, 2, 9, 3, 20)])
def test_references_agree_conv(B, H, W, Cin, Cout):
    rng = np.random.RandomState(B + 10 * H + 100 * W)
    x, dy, w = relu_like(rng, (B, H, W, Cin)), dy_like(rng, (B, H, W, Cout)), he_like(rng, Cin, Cout)
    x64, dy64, w64 = x.astype(np.float64), dy.astype(np.float64), w.astype(np.float64)
    dx = dgrad64(dy64, w64)
    dw, db = wgrad64(x64, dy64)
    assert np.abs(dx).max() > 0 and np.abs(dw).max() > 0
    for a, b in ((dx, dgrad_torch(dy, w)), (dw, wgrad_torch(x, dy)[0]), (db, wgrad_torch(x, dy)[1])):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), (a.shape, np.abs(a - b).max())
    # the float32 yardsticks restate the same sums: within the rigorous float32 bound of the float64 ones
    f_dx, (f_dw, f_db) = dgrad32(dy, w), wgrad32(x, dy)
    a_dw, a_db = wgrad64(np.abs(x64), np.abs(dy64))
    assert (np.abs(f_dx - dx) <= 9 * Cout * U * dgrad64(np.abs(dy64), np.abs(w64))).all()
    assert (np.abs(f_dw - dw) <= B * H * W * U * a_dw).all() and (np.abs(f_db - db) <= B * H * W * U * a_db).all()


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 2, 4), (1, 7, 10, 8), (2, 6, 5, 12)])
def test_references_agree_pool(B, H, W, C):
    rng = np.random.RandomState(H * W + C)
    n = B * H * W * C
    # a permutation of distinct non-zero values, about half negative: no tie inside a window (torch's tie rule is not TF's)
    y = ((rng.permutation(n) - n // 2 + 0.25) / n).reshape(B, H, W, C)
    dpool = rng.standard_normal((B, H // 2, W // 2, C))
    ref = maxpool_backward64(y, dpool)
    assert np.array_equal(ref, maxpool_backward_torch(y, dpool))
    assert ref.any() and not ref[:, 2 * (H // 2):].any() and not ref[:, :, 2 * (W // 2):].any()


def test_shape_tables_reach_every_path(lib):
    """Classifies the tables with rpn_conv3x3_dgrad_tile_n and rpn_conv3x3_wgrad_wide_workspace_bytes, so that a later change of a
    tile rule cannot silently empty a class."""
    for tile in (64, 128):
        shapes = [s for s in DGRAD if lib.rpn_conv3x3_dgrad_tile_n(s[0], s[1], s[2], s[3]) == tile]
        assert shapes, tile
        assert any(s[3] % tile for s in shapes), ("no ragged N tile", tile)
        assert any((s[0] * s[1] * s[2]) % 128 for s in shapes), ("no ragged pixel tile", tile)
        assert any(s[3] % tile == 0 for s in shapes), ("no full N tile", tile)
    small = [s for s in DGRAD if lib.rpn_conv3x3_dgrad_tile_n(s[0], s[1], s[2], s[3]) == 64]
    assert any(s[0] * s[1] * s[2] < 128 for s in small) and any(s[3] < 64 for s in small)
    assert {s[4] for s in DGRAD} >= {16, 48}                     # a new tap at every K slice; tap boundaries off the 64 grid
    assert all(lib.rpn_conv3x3_dgrad_tile_n(s[0], s[1], s[2], s[3]) in (64, 128) for s in DGRAD)
    assert sum(s[1] != s[2] for s in DGRAD) >= 6

    leaves = {s: wide_leaves(lib, *s) for s in WGRAD_WIDE}
    values = set(leaves.values())
    assert 1 in values and 2 in values, leaves                   # wgrad_wide_finish_kernel alone; the tree loop skipped
    assert any(4 <= v <= 64 for v in values) and any(v >= 256 for v in values), leaves
    assert any(s[3] == 3 and v == 1 for s, v in leaves.items()) and any(s[3] == 3 and v >= 256 for s, v in leaves.items()), leaves
    assert any(s[4] % 128 for s in WGRAD_WIDE) and any(s[4] % 128 == 0 for s in WGRAD_WIDE)          # ragged / full Cout tile
    assert {s[3] for s in WGRAD_WIDE} >= {3, 4, 12}
    assert any((9 * s[3]) % 128 == 0 for s in WGRAD_WIDE) and any((9 * s[3]) % 128 for s in WGRAD_WIDE)   # where the ones row lands
    assert sum(s[1] != s[2] for s in WGRAD_WIDE) >= 5

    assert any(s[0] * s[1] * s[2] < 4 for s in WGRAD_HEAD) and any(s[2] < 16 and s[1] > 1 for s in WGRAD_HEAD)
    assert any(s[4] % 128 for s in WGRAD_HEAD) and any(s[4] == 512 for s in WGRAD_HEAD)
    for s in WGRAD_HEAD:
        assert lib.rpn_conv3x3_wgrad_workspace_bytes(*s) > 0, s
    assert any(s[1] % 2 for s in POOL) and any(s[2] % 2 for s in POOL) and any(s[1] != s[2] for s in POOL)


# ---- GPU: guard bands ---------------------------------------------------------------------------------------------------------------------------
class Band:
    """n floats, 16-byte aligned, inside a device buffer whose every other word -- and, without data, every word -- is `canary`
    (CANARY unless a buffer is also read as float64: see test_gpu_backward_mnv2.py)."""

    def __init__(self, n, data=None, canary=CANARY):
        assert n >= 1
        self.n = n
        self.canary = canary
        self.buf = torch.full((n + 2 * GUARD,), canary, dtype=torch.int32, device="cuda")
        self.view = self.buf[GUARD:GUARD + n].view(torch.float32)
        assert self.view.data_ptr() % 16 == 0
        if data is not None:
            assert data.size == n
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(-1)))

    @property
    def ptr(self):
        return L.ptr(self.view)

    def intact(self):
        return bool((self.buf[:GUARD] == self.canary).all()) and bool((self.buf[GUARD + self.n:] == self.canary).all())

    def numpy(self, shape):
        return self.view.cpu().numpy().reshape(shape)


def settle(bands, outputs):
    torch.cuda.synchronize()
    for name, band in bands.items():
        assert band.intact(), "the canary around %s changed: a store outside a buffer" % name
    for name in outputs:
        assert not bool(torch.isnan(bands[name].view).any()), \
            "NaN in %s: an element nobody wrote, or a read outside an input / of workspace nobody wrote" % name


def same_bytes(runs):
    for later in runs[1:]:
        for a, b in zip(runs[0], later):
            assert a.tobytes() == b.tobytes(), "two runs of the same call differ"
    return runs[0]


def workspace(nbytes):
    assert nbytes > 0 and nbytes % 16 == 0
    return Band(nbytes // 4)


def run_dgrad(lib, dy, w, mask=None, runs=2):
    B, H, W, Cout = dy.shape
    Cin = w.shape[2]
    need = lib.rpn_conv3x3_dgrad_workspace_bytes(Cin, Cout)
    bands = {"dy": Band(dy.size, dy), "w": Band(w.size, w)}
    if mask is not None:
        bands["mask"] = Band(mask.size, mask)
    got = []
    for _ in range(runs):
        bands["ws"], bands["dx"] = workspace(need), Band(B * H * W * Cin)
        L.check(lib.rpn_conv3x3_dgrad(bands["dy"].ptr, bands["w"].ptr, bands["mask"].ptr if mask is not None else None, B, H, W, Cin,
                                      Cout, bands["dx"].ptr, bands["ws"].ptr, need, L.stream_ptr()), "rpn_conv3x3_dgrad")
        settle(bands, ("dx",))
        got.append((bands["dx"].numpy((B, H, W, Cin)),))
    return same_bytes(got)[0]


def run_wgrad(lib, wide, x, dy, with_db=True, runs=2):
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    size_fn, fn = (lib.rpn_conv3x3_wgrad_wide_workspace_bytes, lib.rpn_conv3x3_wgrad_wide) if wide else \
        (lib.rpn_conv3x3_wgrad_workspace_bytes, lib.rpn_conv3x3_wgrad)
    need = size_fn(B, H, W, Cin, Cout)
    bands = {"x": Band(x.size, x), "dy": Band(dy.size, dy)}
    got = []
    for _ in range(runs):
        bands["ws"], bands["dw"] = workspace(need), Band(9 * Cin * Cout)
        if with_db:
            bands["db"] = Band(Cout)
        L.check(fn(bands["x"].ptr, bands["dy"].ptr, B, H, W, Cin, Cout, bands["dw"].ptr, bands["db"].ptr if with_db else None,
                   bands["ws"].ptr, need, L.stream_ptr()), "rpn_conv3x3_wgrad_wide" if wide else "rpn_conv3x3_wgrad")
        settle(bands, ("dw", "db") if with_db else ("dw",))
        got.append((bands["dw"].numpy((3, 3, Cin, Cout)),) + ((bands["db"].numpy((Cout,)),) if with_db else ()))
    first = same_bytes(got)
    return first if with_db else (first[0], None)


def run_pool_backward(lib, y, dpool, runs=2):
    B, H, W, C = y.shape
    bands = {"y": Band(y.size, y), "dpool": Band(dpool.size, dpool)}
    got = []
    for _ in range(runs):
        bands["dy_out"] = Band(y.size)
        L.check(lib.rpn_maxpool2x2_backward(bands["y"].ptr, bands["dpool"].ptr, B, H, W, C, bands["dy_out"].ptr, L.stream_ptr()),
                "rpn_maxpool2x2_backward")
        settle(bands, ("dy_out",))
        got.append((bands["dy_out"].numpy((B, H, W, C)),))
    return same_bytes(got)[0]


# ---- GPU: integers, bit-exact over the whole tables (every element compared) -------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout", DGRAD)
def test_dgrad_integers_bit_exact_inside_guard_bands(lib, B, H, W, Cin, Cout):
    rng = np.random.RandomState(B * H + W + Cin)
    # |dy|, |w| <= 2: every partial sum stays below 4 * 9 * Cout <= 4 * 9 * 256 < 2^24 -- exact in float32 whatever the order
    dy = rng.randint(-2, 3, size=(B, H, W, Cout)).astype(np.float32)
    w = rng.randint(-2, 3, size=(3, 3, Cin, Cout)).astype(np.float32)
    mask = rng.choice(np.array([-1.5, -0.0, 0.0, 0.5, 2.0], np.float32), size=(B, H, W, Cin))       # the rule is mask > 0
    ref = dgrad64(dy.astype(np.float64), w.astype(np.float64))
    for use_mask in (False, True):
        got = run_dgrad(lib, dy, w, mask if use_mask else None)
        want = np.where(mask > 0, ref, 0.0) if use_mask else ref
        assert np.array_equal(got, want.astype(np.float32)), use_mask


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout", WGRAD_WIDE)
def test_wgrad_wide_integers_bit_exact_inside_guard_bands(lib, B, H, W, Cin, Cout):
    rng = np.random.RandomState(B + H + W + Cin)
    # |x|, |dy| <= 2: |partial sums| <= 4 * B H W <= 4 * 500 000 < 2^24
    x = rng.randint(-2, 3, size=(B, H, W, Cin)).astype(np.float32)
    dy = rng.randint(-2, 3, size=(B, H, W, Cout)).astype(np.float32)
    dw, db = run_wgrad(lib, True, x, dy)
    ref_w, ref_b = wgrad64(x.astype(np.float64), dy.astype(np.float64))
    assert np.array_equal(dw, ref_w.astype(np.float32))
    assert np.array_equal(db, ref_b.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("B,H,W,Cin,Cout", WGRAD_HEAD)
def test_wgrad_integers_bit_exact_inside_guard_bands(lib, B, H, W, Cin, Cout, with_db):
    rng = np.random.RandomState(B * 7 + W + Cin)
    # |x|, |dy| <= 4: |partial sums| <= 16 * B H W <= 16 * 7688 < 2^24
    x = rng.randint(-4, 5, size=(B, H, W, Cin)).astype(np.float32)
    dy = rng.randint(-4, 5, size=(B, H, W, Cout)).astype(np.float32)
    dw, db = run_wgrad(lib, False, x, dy, with_db)
    ref_w, ref_b = wgrad64(x.astype(np.float64), dy.astype(np.float64))
    assert np.array_equal(dw, ref_w.astype(np.float32))
    assert db is None or np.array_equal(db, ref_b.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["integers", "relu"])
@pytest.mark.parametrize("B,H,W,C", POOL)
def test_maxpool_backward_bit_exact_inside_guard_bands(lib, B, H, W, C, content):
    """The pool backward only routes values, so real-valued data must come out bit-exact too."""
    rng = np.random.RandomState(H + W + C + B)
    if content == "integers":
        # small integers: many positive ties inside a window (the first-max rule), zeros (all-zero windows), negatives
        y = rng.randint(-1, 3, size=(B, H, W, C)).astype(np.float32)
        y[:, :8, :8] = 0.0                                                  # all-zero windows
        y[:, 8:10, 8:10] = 2.0                                              # a window of four equal positive maxima
        y[:, 10:12, 10:12] = -1.0                                           # a window of negatives
    else:
        y = relu_like(rng, (B, H, W, C))                                    # what the trainer keeps: ties only at zero
    dpool = rng.standard_normal((B, H // 2, W // 2, C)).astype(np.float32)
    got = run_pool_backward(lib, y, dpool)
    ref = maxpool_backward64(y.astype(np.float64), dpool.astype(np.float64))
    assert np.array_equal(got, ref.astype(np.float32))
    assert not got[:, 2 * (H // 2):].any() and not got[:, :, 2 * (W // 2):].any()           # the uncovered row and column
    if content == "integers" and H >= 12 and W >= 12:
        assert got[:, 8, 8].any() and not got[:, 8, 9].any() and not got[:, 9, 8].any() and not got[:, 9, 9].any()
        assert not got[:, :8, :8].any() and not got[:, 10:12, 10:12].any()


# ---- GPU: real values against float64 ---------------------------------------------------------------------------------------------------------
def parity(what, shape, got, ref, f32, absprod, K, depth):
    """err(gpu) <= MARGIN * max(e32, 2^-24) and |got - ref| <= (K + depth) 2^-24 (|A| |B|) element-wise; prints the two errors."""
    scale = np.abs(ref).max()
    assert scale > 0, (what, shape)
    d = np.abs(got - ref)
    e_gpu, e32 = d.max() / scale, np.abs(f32 - ref).max() / scale
    print("parity %-12s %-26s err_gpu %.2e  e32 %.2e  ratio %.2f" % (what, shape, e_gpu, e32, e_gpu / max(e32, U)))
    assert e_gpu <= MARGIN * max(e32, U), (what, shape, e_gpu, e32)
    assert (d <= (K + depth) * U * absprod).all(), (what, shape, "beyond the rigorous float32 bound")


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout", DGRAD)
def test_dgrad_real_values_match_float64(lib, B, H, W, Cin, Cout):
    for seed in range(1000 + B * H + W + Cin, 1032 + B * H + W + Cin):
        rng = np.random.RandomState(seed)
        dy, w, mask = dy_like(rng, (B, H, W, Cout)), he_like(rng, Cin, Cout), relu_like(rng, (B, H, W, Cin))
        dy64, w64 = dy.astype(np.float64), w.astype(np.float64)
        ref = dgrad64(dy64, w64)
        if ref.any() and ref[mask > 0].any():    # a one-pixel case can draw an all-zero dy or an all-zero mask
            break
    f32, absprod = dgrad32(dy, w), dgrad64(np.abs(dy64), np.abs(w64))
    shape = (B, H, W, Cin, Cout)
    parity("dgrad dx", shape, run_dgrad(lib, dy, w), ref, f32, absprod, 9 * Cout, 0)
    keep = mask > 0
    got = run_dgrad(lib, dy, w, mask)
    assert not got[~keep].any()
    parity("dgrad masked", shape, got, np.where(keep, ref, 0.0), np.where(keep, f32, np.float32(0)), np.where(keep, absprod, 0.0),
           9 * Cout, 0)


def wgrad_parity(lib, wide, shape, with_db, depth):
    B, H, W, Cin, Cout = shape
    for seed in range(2000 + B + H + W + Cin + Cout, 2032 + B + H + W + Cin + Cout):
        rng = np.random.RandomState(seed)
        x, dy = relu_like(rng, (B, H, W, Cin)), dy_like(rng, (B, H, W, Cout))
        x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
        ref_w, ref_b = wgrad64(x64, dy64)
        if ref_w.any() and ref_b.any():         # half of x and of dy is zero: one or two pixels can draw an all-zero gradient
            break
    (f_w, f_b), (abs_w, abs_b) = wgrad32(x, dy), wgrad64(x64, np.abs(dy64))     # x >= 0 already
    dw, db = run_wgrad(lib, wide, x, dy, with_db)
    name = "wgrad_wide" if wide else "wgrad"
    parity(name + " dw", shape, dw, ref_w, f_w, abs_w, B * H * W, depth)
    if with_db:
        parity(name + " db", shape, db, ref_b, f_b, abs_b, B * H * W, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout", WGRAD_WIDE)
def test_wgrad_wide_real_values_match_float64(lib, B, H, W, Cin, Cout):
    leaves = wide_leaves(lib, B, H, W, Cin, Cout)
    wgrad_parity(lib, True, (B, H, W, Cin, Cout), True, int(math.log2(leaves)))


@pytest.mark.gpu
@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("B,H,W,Cin,Cout", WGRAD_HEAD)
def test_wgrad_real_values_match_float64(lib, B, H, W, Cin, Cout, with_db):
    wgrad_parity(lib, False, (B, H, W, Cin, Cout), with_db, 2)                # four leaves: (l0 + l1) + (l2 + l3)


# ---- GPU: one chained block boundary at full size ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w,H,W", [(2, 125, 125, 250, 250), (2, 125, 97, 250, 194), (1, 125, 125, 251, 250)])
def test_block_boundary_chain_matches_float64(lib, B, h, w, H, W):
    """block3_conv1 -> block2_pool -> block2_conv2 as backbone_backward chains them: dgrad without mask, the pool backward (+ the
    ReLU mask of the pooled conv), the wide wgrad of block2_conv2.  The float64 chain routes through the same float32 y, so no pool
    maximum flips and the bound is the single-layer one."""
    rng = np.random.RandomState(3000 + B + w + H)
    dy3, w3 = dy_like(rng, (B, h, w, 256)), he_like(rng, 128, 256)
    y2, x2 = relu_like(rng, (B, H, W, 128)), relu_like(rng, (B, H, W, 128))         # block2_conv2's output and input
    shape = (B, h, w, H, W)
    r1 = dgrad64(dy3.astype(np.float64), w3.astype(np.float64))
    r2 = maxpool_backward64(y2.astype(np.float64), r1)
    r_w, r_b = wgrad64(x2.astype(np.float64), r2)
    f1 = dgrad32(dy3, w3)
    f2 = maxpool_backward64(y2, f1).astype(np.float32)                              # routing only: exact
    f_w, f_b = wgrad32(x2, f2)

    def chain_parity(what, got, ref, f32):
        scale = np.abs(ref).max()
        e_gpu, e32 = np.abs(got - ref).max() / scale, np.abs(f32 - ref).max() / scale
        print("parity %-12s %-26s err_gpu %.2e  e32 %.2e  ratio %.2f" % (what, shape, e_gpu, e32, e_gpu / max(e32, U)))
        assert e_gpu <= MARGIN * max(e32, U), (what, shape, e_gpu, e32)

    g1 = run_dgrad(lib, dy3, w3, runs=1)
    chain_parity("chain dgrad", g1, r1, f1)
    g2 = run_pool_backward(lib, y2, g1, runs=1)
    assert not g2[:, 2 * h:].any() and not g2[:, :, 2 * w:].any()
    assert np.array_equal(g2, maxpool_backward64(y2, g1).astype(np.float32))          # the pool step alone is exact
    chain_parity("chain pool", g2, r2, f2)
    dw, db = run_wgrad(lib, True, x2, g2, runs=1)
    chain_parity("chain dw", dw, r_w, f_w)
    chain_parity("chain db", db, r_b, f_b)
